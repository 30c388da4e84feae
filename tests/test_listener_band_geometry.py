"""The HIP path against the CPU oracle, bit for bit, at the listener and band counts where the hot path switches code:

  512 / 513 slots at N = 16384   k_fft_r32 (and its wide tap, read by k_cum_refine) or the 16-point k_fft_psd<14>
  4096 / 4097 listeners          the one-frame FFT kernel's LDS tap or its drain path
  many gather rows               k_listen_gather's grid.y = ceil(n_slots / 64), decoder groups of 16
  many bands                     grid.y = n_bands in the FFT kernels, k_fft_r32's per-band claim counters, 64 bands of
                                 config 5 on one GPU (eager and as graph replays)
  the small plan                 B * N <= 8192: the gather on the peaks stream, behind many sdr_attach_at slot writes

and across the transitions between them inside one stream: the slot pool is a high-water mark, so the 513th listener
moves a bank off k_fft_r32 for good, with cumulation and decoder state carried over, and a listener bound with
sdr_attach_at inside a deferred batch can make that move between the batch's FFT and its listen half.

Listeners beyond the keyed carriers sit on bins 0 and N - 1 (the wide tap's wrap-around neighbours), beside carriers
(the wide tap stores bin - 1 and bin + 1), on a carrier a second time and on noise bins.  The oracle runs every band
segment by segment, with each attach and detach at the frame where the bank applies it; its outputs are stitched into
one stream per band (a listener's keying column is zero before it is attached) and compared with what sdr_poll
delivers and what stays on the device: frame records, keying bits, edges, runes, decoder state, the exact cumulation
rows (and the kept row: never below the exact one, equal at and beside every peak) and peaks.
"""
import pytest

from parity_case import RATE, Case
from parity_tools import capi  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu


# -- 1. N = 16384 at 512 and 513 slots -----------------------------------------------------------------------------------

@pytest.mark.parametrize("slots", [512, 513])
def test_fft_r32_slot_limit(capi, slots):
    """N = 16384, 256 keyed carriers and `slots` listeners, two 1024-frame batches (n_frames * n_bands >= 1024, so the
    frame count alone would pick k_fft_r32).  fft_choice (host/batch_plan.h, `tap_n <= kR32MaxTap`) selects k_fft_r32 at
    512 slots - register tap, wide tap and tap_used written, and k_cum_refine reading them (capi_process.hip issue_cumulation,
    FftChoice::wide_tap) - and the one-frame k_fft_psd<14> with its LDS tap at 513, where k_cum_refine reads the psd.
    max_listeners is 600 in both, so tap_stride > 512 and the tap_used entries past 512 exist.  513 slots also need a
    ninth gather row (k_listen.hip:709, grid.y = (n_slots + 63) / 64)."""
    c = Case(16384, 1, 256, slots, [("batch", 1024), ("batch", 1024)], seed=6100 + slots, max_listeners=600)
    c.run(capi).close()


# -- 2. crossing 512 slots inside a stream ---------------------------------------------------------------------------------

def test_crossing_512_slots_by_attach_then_holes(capi):
    """N = 16384: a 1024-frame batch at 512 slots (k_fft_r32, host/batch_plan.h fft_choice), sdr_attach of a 513th
    listener, a batch at 513 slots (k_fft_psd<14>: the pool is a high-water mark, capi_bank.hip:421), then three listeners
    detached - holes under the high-water mark, still 513 slots and still k_fft_psd<14> - and a third batch.  The
    cumulation and every decoder run across both switches."""
    steps = [("batch", 1024), ("attach", 0, 9000), ("batch", 1024),
             ("detach", 0, 5), ("detach", 0, 300), ("detach", 0, 511), ("batch", 1024)]
    c = Case(16384, 1, 256, 512, steps, seed=6200, max_listeners=600)
    c.run(capi).close()


def test_crossing_512_slots_inside_a_deferred_batch(capi):
    """N = 16384: a deferred 1024-frame batch whose FFT runs at 512 slots (k_fft_r32, wide tap), then sdr_attach_at
    binds listeners 513 and 514 at the cumulation boundaries 300 and 700 inside it, so its listen half gathers 514 slots
    (k_listen.hip:709, a ninth gather row; k_listen.hip:67, frames before tapped_from from the retained psd rows); the
    next deferred batch runs k_fft_psd<14> (host/batch_plan.h fft_choice: tap_n > kR32MaxTap) with every listener on the tap."""
    steps = [("defer", 1024, [(0, 4000, 300), (0, 9001, 700)]), ("defer", 1024, [])]
    c = Case(16384, 1, 256, 512, steps, seed=6300, max_listeners=600)
    c.run(capi).close()


# -- 3. kMaxLdsTap ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,listeners", [(8192, 4096), (8192, 4097), (16384, 4100)])
def test_lds_tap_capacity(capi, n, listeners):
    """The one-frame FFT kernel (host/batch_plan.h kDefaultFpw = 1) keeps its listeners' bins in LDS while
    n_tap <= kMaxLdsTap (k_fft_psd.h `lds_tap`, and the dynamic LDS size in launch_fft_t) and drains the tap from the
    stored psd row past it (:635, tap_frame).  4096 and 4097 listeners on one band of N = 8192 in two 512-frame batches,
    and 4100 at N = 16384 in two 1024-frame batches: the frame count would select k_fft_r32 there, and it is the slot
    count (fft_choice, tap_n > kR32MaxTap) that puts the tap on k_fft_psd<14> instead.  64 or 65 gather rows."""
    frames = 1024 if n == 16384 else 512
    c = Case(n, 1, 256, listeners, [("batch", frames), ("batch", frames)], seed=6400 + listeners)
    c.run(capi).close()


# -- 4. many bands --------------------------------------------------------------------------------------------------------------

def test_config5_whole_on_one_gpu(capi):
    """BASELINE config 5 whole on one GPU: 64 bands x N = 8192 x 16 listeners (1024 in all): grid.y = 64 in the FFT
    and noise kernels, 64 bands of frame records and ListenGeom frame bases.  Six eager 24-frame batches (capture needs
    the bank at a multiple of sdr_graph_batches(); the fifth straddles the cumulation boundary at frame 99), then one
    graph replay (capi_graph.hip:118 sdr_graph_capture, :237 sdr_graph_launch) of six more (the boundary at 199 inside
    its third batch).  Every band against its own oracle receiver."""
    import torch

    per = 24
    c = Case(8192, 64, 16, 16, [("batch", per)] * 12, seed=6500, free_last=False)
    c.run_oracle()
    bank = c.new_bank(capi, torch.cuda.Stream())
    K = bank.graph_batches
    assert K * per * 2 == c.total
    for k in range(K):
        a, e = k * per, (k + 1) * per
        batch = c.device_batch(a, e)
        torch.cuda.synchronize()  # (the input is written on torch's stream, the bank reads it on its own)
        bank.process_device(batch.data_ptr(), per)
        res = bank.poll(wait=True)
        assert res["batch_index"] == k
        c.check_polled(res, a, e)
        c.check_device(bank, a, e, k)
    bank.graph_capture(per)
    batches = [c.device_batch((K + k) * per, (K + k + 1) * per) for k in range(K)]
    torch.cuda.synchronize()
    bank.graph_launch([x.data_ptr() for x in batches])
    for k in range(K):
        res = bank.poll(wait=True)
        a = (K + k) * per
        assert res["batch_index"] == K + k
        c.check_polled(res, a, a + per)
    bank.sync()
    assert bank.total_frames == c.total
    c.check_device(bank, c.total - per, c.total, 2 * K - 1, cumulations=False)
    c.check_end(bank, min_edges=8)
    bank.close()


def test_fft_r32_claim_counters_beyond_8_bands(capi):
    """k_fft_r32 on 24 bands x N = 16384 x 64-frame batches (host/batch_plan.h fft_choice: 64 * 24 >= 1024 frames per
    launch, 16 slots): a claim counter pair per band (k_fft_r32.hip:289 `steal + 2 * blockIdx.y`), put back to zero by
    each band's last workgroup (:574), over two launches."""
    c = Case(16384, 24, 16, 16, [("batch", 64), ("batch", 64)], seed=6600, free_last=False)
    c.run(capi, min_edges=5).close()


# -- 5. the small plan behind many late attaches ------------------------------------------------------------------------------

@pytest.mark.parametrize("n,n_bands,rate,early,late", [(8192, 1, RATE, 32, 320), (4096, 2, 192_000, 16, 200)])
def test_small_plan_many_late_attaches(capi, n, n_bands, rate, early, late):
    """B * N <= 8192 (host/batch_plan.h plan_batch's gather stream: the gather on the peaks stream): one deferred 1000-frame
    batch in which sdr_attach_at binds `late` listeners per band at the nine cumulation boundaries inside it - dozens of
    k_put_slots launches on the listen stream (capi_process.hip flush_late_attached) - then two eager batches with every
    listener carried.  Each batch is polled only after the next one is enqueued, so the listen stream may still be
    behind when the next gather is issued on the peaks stream; every such gather waits for the last put until the host
    has seen it done (slots_put_ev in capi_process.hip issue_listen).  The oracle attaches each listener at its frame."""
    boundaries = list(range(100, 1000, 100))

    def steps(carriers):
        # the late listeners are the carriers after the first `early`, bound boundary by boundary, band by band
        late_steps = [(b, carriers[b][early + j], boundaries[j * len(boundaries) // late]) for b in range(n_bands) for j in range(late)]
        return [("defer", 1000, sorted(late_steps, key=lambda t: (t[2], t[0]))), ("batch", 1000), ("batch", 1000)]

    c = Case(n, n_bands, early + late, early, steps, seed=6700 + n, rate=rate, total_frames=3000)
    c.run(capi, lag=True).close()
