"""Run by tests/test_fft_reserve_gpu.py in a process of its own (the number of hardware queues is fixed when the runtime
starts): one bank of N = 16384 on a torch stream, one 2048-frame batch of pooled frames, the psd rows of a few frames
printed as a hash.  The library's queue probe reports on stderr (SDR_QUEUE_DEBUG=1)."""
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sdrainer_amd import capi  # noqa: E402
from parity_tools import POOL_N as N, pool_bank, pool_batch, pool_frames  # noqa: E402

capi.load()
frames = 2048
iq, want = pool_frames(7700)
bank = pool_bank(capi, 1, frames)
stream = torch.cuda.Stream()
bank.set_stream(stream.cuda_stream)
dev = pool_batch(torch.from_numpy(iq).cuda(), frames)
torch.cuda.synchronize()
for _ in range(2):
    bank.process_device(dev.data_ptr(), frames)
bank.sync()
h = hashlib.sha256()
psd = np.empty(N, np.float32)
bad = 0
for f in (0, 1, 60, 61, 1000, 2047):
    assert bank._L.sdr_read_spectrum(bank._h, 0, f, None, C.c_void_p(psd.ctypes.data)) == 0
    bad += not np.array_equal(psd.view(np.uint32), want[f % 61])
    h.update(psd.tobytes())
bank.close()
print("rows differing from the oracle: %d, hash %s" % (bad, h.hexdigest()[:16]))
