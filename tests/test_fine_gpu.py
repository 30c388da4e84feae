"""The fine converter on the GPU (sdr_fine_*, csrc/k_fine.hip) against its NumPy restatement tests/fine_ref.py, bit for bit:
the decimations and tap counts at which the kernel's tile takes another shape, with several bands on one input and one input
unread; the limits of 64 bands and 256 inputs; cuts of the streams into calls; the step and the input map changed between
calls; sample indices across 2^31 and 2^32; every band against a one-band SDR_DDC_F32 down-converter on the GPU; a stream
switch; subnormal products; every refusal; and the chain - one cu8 wide stream through channelizer, fine converter and bank
on one HIP stream, cut into whole hops and cut raggedly - against the oracle receiver fed with the reference chain's narrow
streams."""
import ctypes as C

import numpy as np
import pytest

import ddc_ref as R
import ddc_run
import fine_ref as F
from fine_run import run_gpu
from parity_tools import bits_equal, capi, check_batch_polled, run_oracle  # noqa: F401

pytestmark = pytest.mark.gpu

STEPS = (0, 9000, -32768, -1)
INPUTS = (2, 0, 2, 0)  # of 3: input 1 is unread


@pytest.fixture(scope="module")
def table(capi):
    return capi.ddc_nco_table()


def random_taps(t, seed):
    return np.random.default_rng(seed).uniform(-1, 1, t).astype(np.float32)


def streams(n_inputs, n, seed):
    return np.stack([R.random_raw(n, R.F32, seed + i) for i in range(n_inputs)])


def cut(x, lens):
    assert sum(lens) == x.shape[1]
    cuts = np.cumsum([0] + list(lens))
    return [x[:, a:e] for a, e in zip(cuts[:-1], cuts[1:])]


@pytest.mark.parametrize("d,t,m", [(1, 1, 5), (3, 7, 23), (8, 64, 513), (64, 1024, 130), (256, 4096, 65), (5, 4, 1030)])
def test_parity_with_the_reference(capi, table, d, t, m):
    """(5, 4, 1030) is two tiles and a tail; (8, 64, 513) a tile and one output; the input stride and the band stride are
    larger than the lengths (fine_run)."""
    taps = random_taps(t, 100 * d + t)
    x = streams(3, d * m, 7 * d + t)
    want = F.fine_ref(x, d, taps, STEPS, *table, inputs=INPUTS)
    got = run_gpu(capi, d, taps, STEPS, INPUTS, [x], in_gap=8, out_gap=12)
    assert got.shape == (len(STEPS), m, 2)
    assert bits_equal(got, want)


def test_the_limits_at_a_tiny_size(capi, table):
    """64 bands from 256 inputs, the map from input 255 downwards."""
    d, t, m = 2, 3, 9
    steps = [int(s) for s in np.random.default_rng(1).integers(-32768, 32768, 64)]
    inputs = [255 - 4 * b for b in range(64)]
    assert inputs[0] == 255 and len(set(inputs)) == 64
    taps = random_taps(t, 2)
    x = streams(256, d * m, 1000)
    want = F.fine_ref(x, d, taps, steps, *table, inputs=inputs)
    assert bits_equal(run_gpu(capi, d, taps, steps, inputs, [x]), want)
    # and cut into calls of one output: every input's carry is kept
    assert bits_equal(run_gpu(capi, d, taps, steps, inputs, cut(x, [d] * m)), want)


@pytest.mark.parametrize("d,t", [(3, 7), (8, 64)])
def test_call_cuts(capi, table, d, t):
    """Calls of one output and of five, two consecutive calls shorter than T - 1 (part of every carry survives each), the rest."""
    taps = random_taps(t, 5)
    short = max(d, (t - 1) // d // 2 * d)
    assert 0 < short < t - 1 and d < t - 1
    lens = [d, 5 * d, short, short, 700 * d]
    x = streams(3, sum(lens), 900)
    want = F.fine_ref(x, d, taps, STEPS, *table, inputs=INPUTS)
    assert bits_equal(run_gpu(capi, d, taps, STEPS, INPUTS, [x]), want)
    assert bits_equal(run_gpu(capi, d, taps, STEPS, INPUTS, cut(x, lens)), want)


def test_step_and_input_changes_between_calls(capi, table):
    """Band 0 moves to input 1, which nobody has read so far, and back; band 3 is retuned; band 1 moves for good."""
    d, t = 8, 64
    taps = random_taps(t, 12)
    lens = [64 * d, 3 * d, 200 * d]
    x = streams(3, sum(lens), 32)
    pieces = cut(x, lens)
    changes = {1: [("set_input", 0, 1), ("set_nco_step", 3, -4000), ("set_input", 1, 2)], 2: [("set_input", 0, 2), ("set_nco_step", 3, 77)]}
    ref = F.FineRef(3, d, taps, STEPS, *table, inputs=INPUTS)
    want = []
    for i, p in enumerate(pieces):
        for name, band, value in changes.get(i, ()):
            getattr(ref, name)(band, value)
        want.append(ref.process(p))
    want = np.concatenate(want, axis=1)

    def between(fine, i):
        for name, band, value in changes.get(i, ()):
            getattr(fine, name)(band, value)

    got = run_gpu(capi, d, taps, STEPS, INPUTS, pieces, between=between)
    assert bits_equal(got, want)
    assert not bits_equal(got, F.fine_ref(x, d, taps, STEPS, *table, inputs=INPUTS))  # (the changes did change the bands)
    # the moved band found input 1's history: its three outputs are a DDC's that read input 1 from the start
    assert bits_equal(got[0, 64:67], R.ddc_ref(x[1], d, taps, (STEPS[0],), *table)[0][64:67])


@pytest.mark.parametrize("edge", [2 ** 31, 2 ** 32], ids=["2^31", "2^32"])
def test_large_sample_index(capi, table, edge):
    """The calls cross k = edge; one band has an odd step and one step -1: the phase comes from the full 64-bit index."""
    d, t, steps, inputs = 8, 24, (12345, -1, 9000), (1, 0, 1)
    taps = random_taps(t, 11)
    k0 = edge - 50 * d
    lens = [40 * d, 40 * d, 30 * d]  # the second call crosses the edge
    x = streams(2, sum(lens), 31)
    want = F.fine_ref(x, d, taps, steps, *table, inputs=inputs, first_sample=k0)
    got = run_gpu(capi, d, taps, steps, inputs, cut(x, lens), first_sample=k0)
    assert bits_equal(got, want)
    # (samples below k0 are zero: the first outputs see fewer than T samples, as at index 0)
    assert bits_equal(got[2][0], (taps[0] * R.mix(x[1, :1], np.array([k0]), 9000, *table))[0])


def test_every_band_equals_a_one_band_ddc_on_the_gpu(capi, table):
    """GPU against GPU: what an SDR_DDC_F32 sdr_ddc of one band makes of the band's stream, under the same cuts."""
    d, t = 5, 40
    taps = random_taps(t, 14)
    lens = [d * 300, d * 3, d * 730]
    x = streams(3, sum(lens), 50)
    got = run_gpu(capi, d, taps, STEPS, INPUTS, cut(x, lens))
    for b, (step, i) in enumerate(zip(STEPS, INPUTS)):
        one = ddc_run.run_gpu(capi, R.F32, d, taps, (step,), [p[i] for p in cut(x, lens)])
        assert bits_equal(got[b], one[0]), b


def test_a_stream_switch_between_calls(capi, table):
    d, t = 8, 64
    taps = random_taps(t, 16)
    lens = [d * 600, d * 5, d * 600]
    x = streams(3, sum(lens), 60)
    want = F.fine_ref(x, d, taps, STEPS, *table, inputs=INPUTS)
    assert bits_equal(run_gpu(capi, d, taps, STEPS, INPUTS, cut(x, lens), switch_at=1), want)


def test_subnormal_products_are_kept(capi, table):
    d, t = 4, 32
    rng = np.random.default_rng(13)
    taps = (rng.uniform(-1, 1, t) * 1e-10).astype(np.float32)
    x = (rng.uniform(-1, 1, (3, d * 600, 2)) * 1e-30).astype(np.float32)
    want = F.fine_ref(x, d, taps, STEPS, *table, inputs=INPUTS)
    tiny = np.finfo(np.float32).tiny
    assert np.all(np.abs(want) < tiny) and np.count_nonzero(want) > want.size * 0.9  # every output is subnormal, few are zero
    assert bits_equal(run_gpu(capi, d, taps, STEPS, INPUTS, [x]), want)


def test_refusals_change_nothing(capi, table):
    import torch

    L = capi.load()
    vp = C.c_void_p
    i32p = C.POINTER(C.c_int32)
    d, t, steps, inputs, n_inputs = 4, 16, (100, -200), (2, 0), 3
    taps = random_taps(t, 15)
    tp = taps.ctypes.data_as(C.POINTER(C.c_float))
    st = np.array(steps, np.int32)
    sp = st.ctypes.data_as(i32p)
    ins = np.array(inputs, np.int32)
    ip = ins.ctypes.data_as(i32p)
    cap = 64 * d

    def config(**kw):
        c = capi.FineConfig(C.sizeof(capi.FineConfig), len(steps), n_inputs, d, t, cap, 0, 0)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def ints(*v):
        a = np.array(v, np.int32)
        keep.append(a)
        return a.ctypes.data_as(i32p)

    keep = []
    h = vp()
    fine = capi.Fine(n_inputs, d, taps, steps, inputs=inputs, max_in_samples=cap)
    fine.set_stream(torch.cuda.current_stream().cuda_stream)
    fine.set_first_sample(8 * d)
    piece, in_stride = 8 * d, 8 * d + 4
    dev = torch.zeros((n_inputs, cap + 8, 2), dtype=torch.float32, device="cuda")
    out = torch.zeros((2, 80, 2), dtype=torch.float32, device="cuda")
    i_ok, o_ok = vp(dev.data_ptr()), vp(out.data_ptr())
    refusals = [
        (capi.ERR_BAD_ARG, L.sdr_fine_create, None, tp, sp, ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config()), None, sp, ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config()), tp, None, ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config()), tp, sp, ip, None),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config(struct_size=28)), tp, sp, ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config(n_bands=0)), tp, sp, ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config(n_bands=65)), tp, sp, ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config(n_inputs=0)), tp, sp, ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config(n_inputs=257)), tp, sp, ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config(decimation=0)), tp, sp, ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config(decimation=257, max_in_samples=257)), tp, sp, ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config(n_taps=0)), tp, sp, ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config(n_taps=4097)), tp, sp, ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config(max_in_samples=cap + 1)), tp, sp, ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config(max_in_samples=0)), tp, sp, ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config(reserved=1)), tp, sp, ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config()), tp, ints(100, 32768), ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config()), tp, ints(-32769, 0), ip, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config()), tp, sp, ints(0, 3), C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config()), tp, sp, ints(-1, 0), C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_fine_create, C.byref(config(n_inputs=1)), tp, sp, None, C.byref(h)),  # no map, more bands than inputs
        (capi.ERR_BAD_ARG, L.sdr_fine_process_device, fine._h, vp(dev.data_ptr() + 8), in_stride, piece, o_ok, 8),   # misaligned input
        (capi.ERR_BAD_ARG, L.sdr_fine_process_device, fine._h, i_ok, in_stride, piece, vp(out.data_ptr() + 8), 8),   # misaligned output
        (capi.ERR_BAD_ARG, L.sdr_fine_process_device, fine._h, None, in_stride, piece, o_ok, 8),
        (capi.ERR_BAD_ARG, L.sdr_fine_process_device, fine._h, i_ok, in_stride, piece, None, 8),
        (capi.ERR_BAD_ARG, L.sdr_fine_process_device, None, i_ok, in_stride, piece, o_ok, 8),
        (capi.ERR_BAD_SIZE, L.sdr_fine_process_device, fine._h, i_ok, in_stride, piece + 1, o_ok, 12),  # not a multiple of D
        (capi.ERR_BAD_SIZE, L.sdr_fine_process_device, fine._h, i_ok, in_stride, 0, o_ok, 8),
        (capi.ERR_BAD_SIZE, L.sdr_fine_process_device, fine._h, i_ok, cap + 8, cap + d, o_ok, 80),      # above the capacity
        (capi.ERR_BAD_ARG, L.sdr_fine_process_device, fine._h, i_ok, piece - 4, piece, o_ok, 8),        # an input stride below the samples
        (capi.ERR_BAD_ARG, L.sdr_fine_process_device, fine._h, i_ok, piece + 2, piece, o_ok, 8),        # not a multiple of 4
        (capi.ERR_BAD_ARG, L.sdr_fine_process_device, fine._h, i_ok, in_stride, piece, o_ok, 4),        # a band stride below the outputs
        (capi.ERR_BAD_ARG, L.sdr_fine_process_device, fine._h, i_ok, in_stride, piece, o_ok, 10),       # not a multiple of 4
        (capi.ERR_BAD_ARG, L.sdr_fine_set_nco_step, fine._h, 2, 5),
        (capi.ERR_BAD_ARG, L.sdr_fine_set_nco_step, fine._h, -1, 5),
        (capi.ERR_BAD_ARG, L.sdr_fine_set_nco_step, fine._h, 0, 32768),
        (capi.ERR_BAD_ARG, L.sdr_fine_set_nco_step, fine._h, 0, -32769),
        (capi.ERR_BAD_ARG, L.sdr_fine_set_nco_step, None, 0, 5),
        (capi.ERR_BAD_ARG, L.sdr_fine_set_input, fine._h, 2, 1),
        (capi.ERR_BAD_ARG, L.sdr_fine_set_input, fine._h, -1, 1),
        (capi.ERR_BAD_ARG, L.sdr_fine_set_input, fine._h, 0, 3),
        (capi.ERR_BAD_ARG, L.sdr_fine_set_input, fine._h, 0, -1),
        (capi.ERR_BAD_ARG, L.sdr_fine_set_input, None, 0, 1),
        (capi.ERR_BAD_ARG, L.sdr_fine_sync, None),
        (capi.ERR_BAD_ARG, L.sdr_fine_set_stream, None, None),
        (capi.ERR_BAD_ARG, L.sdr_fine_set_first_sample, None, 0),
        (capi.ERR_STATE, L.sdr_fine_set_first_sample, fine._h, 16 * d),  # (after the first good call, below)
    ]
    assert L.sdr_fine_set_first_sample(fine._h, -d) == capi.ERR_BAD_ARG and L.sdr_fine_set_first_sample(fine._h, 8 * d + 1) == capi.ERR_BAD_ARG
    assert fine.total_samples == 8 * d and L.sdr_fine_total_samples(None) == 0 and L.sdr_fine_destroy(None) == capi.OK
    # a good call of 8 outputs in front of the first refusal and behind every one: the streams go on as if nothing was tried
    x = streams(n_inputs, piece * (len(refusals) + 1), 16)
    want = F.fine_ref(x, d, taps, steps, *table, inputs=inputs, first_sample=8 * d)
    for i in range(len(refusals) + 1):
        if i:
            status, call, *args = refusals[-i]
            h.value = 0xdead
            assert call(*args) == status, (i, L.sdr_last_error())
            assert h.value == 0xdead and L.sdr_last_error()
            assert fine.total_samples == 8 * d + i * piece
        dev[:, :piece] = torch.from_numpy(x[:, i * piece:(i + 1) * piece]).cuda()
        fine.process_device(dev.data_ptr(), cap + 8, piece, out.data_ptr(), 80)
        fine.sync()
        assert bits_equal(out.cpu().numpy()[:, :8], want[:, 8 * i:8 * i + 8]), f"the good call behind refusal {i}"
    fine.close()


# -- the chain: cu8 wide stream -> channelizer -> fine converter -> bank ------------------------------------------------------
@pytest.fixture(scope="module")
def e2e(table):
    """The fixture through the reference chain and the oracle receiver, once for both tests."""
    e = F.E2E
    raw, narrow, one, two = F.e2e_reference(*table)
    centers = [14_000_000 + int(round(t * e["wide_rate"] / (F.L * e["d1"]))) for t in e["targets"]]
    _, outs, decs = run_oracle(e["rate"], e["n"], e["edge"], [[b] for b in e["bins"]], list(two), centers, e["hop"])
    return raw, narrow, one, two, centers, outs, decs


def ragged_lengths(narrow, hop):
    """Call lengths in narrow outputs, drawn with a fixed seed, as a receiver's are: each even (the next call's pointers stay
    16-byte aligned), none a multiple of the hop, a third of them shorter than a hop - after which the bank often has no
    whole new frame."""
    rng = np.random.default_rng(20_241)
    lens, left = [], narrow
    while left > 0:
        m = 2 * int(rng.integers(1, hop // 2) if rng.random() < 0.35 else rng.integers(hop, 100 * hop))
        m += 2 * (m % hop == 0)
        lens.append(min(m, left))
        left -= lens[-1]
    assert all(m % 2 == 0 for m in lens) and all(m % hop for m in lens[:-1]) and sum(lens) == narrow
    return lens


def chain(capi, e2e, lens=None):
    """Channelizer (M = 8, D = 4), fine converter (D = 8, the steps and channels sdr_fine_tune names) and bank (N = 512, hop
    128, sdr_process_device_stream) on one HIP stream: call triples back to back with no host synchronisation inside a
    triple and one at the end.  lens: the narrow outputs per triple (by default 512 frames' worth each), so a stage-one call
    is a multiple of D1 * D2 wide samples; the bank takes whatever whole frames exist and is skipped where there is none.
    Stage one's band stride is stage two's input stride: nothing is copied."""
    import torch

    e = F.E2E
    n, hop, rate, frames, d1, d2 = e["n"], e["hop"], e["rate"], e["frames"], e["d1"], e["d2"]
    raw, narrow, one, two, centers, outs, decs = e2e
    h1, h2 = F.e2e_taps()
    tuned = [capi.fine_tune(e["n_channels"], d1, t) for t in e["targets"]]
    assert tuple(c for c, _ in tuned) == e["channels"] and tuple(s for _, s in tuned) == e["fine_steps"]
    per = 512  # frames' worth of narrow samples per triple, at the most
    if lens is None:
        lens = [min(per * hop, narrow - a) for a in range(0, narrow, per * hop)]
    assert sum(lens) == narrow and max(lens) <= per * hop
    mid_stride, stride = narrow * d2, narrow
    assert stride % 4 == 0
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        wide = torch.from_numpy(raw.copy()).cuda()  # (the shared fixture is read-only)
        mid =torch.full((2, mid_stride, 2), float("nan"), dtype=torch.float32, device="cuda")
        out = torch.full((2, stride, 2), float("nan"), dtype=torch.float32, device="cuda")
    stream.synchronize()
    bank = capi.Bank(rate, n, n_bands=2, edge_width=e["edge"], max_batch_frames=per, max_listeners=2, hop=hop)
    chan = capi.Chan(e["n_channels"], d1, h1, [c for c, _ in tuned], in_format=capi.DDC_CU8, max_in_samples=per * hop * d1 * d2)
    fine = capi.Fine(2, d2, h2, [s for _, s in tuned], max_in_samples=per * hop * d2)
    for obj in (bank, chan, fine):
        obj.set_stream(stream.cuda_stream)
    for b in range(2):
        bank.set_center_frequency(b, centers[b])
        assert bank.attach(b, e["bins"][b]) == 0
    bank.enable_results(True)
    have = done = skipped = 0  # narrow samples produced, frames processed, triples in which the bank had no new frame
    batches = []
    for k in lens:
        chan.process_device(wide.data_ptr() + have * d1 * d2 * 2, k * d1 * d2, mid.data_ptr() + have * d2 * 8, mid_stride)
        fine.process_device(mid.data_ptr() + have * d2 * 8, mid_stride, k * d2, out.data_ptr() + have * 8, stride)
        have += k
        f = (have - n) // hop + 1 - done if have >= n else 0
        if f == 0:
            skipped += 1
            continue
        bank.process_device_stream(out.data_ptr() + done * hop * 8, f, stride)
        batches.append((done, done + f))
        done += f
    chan.sync()
    fine.sync()
    bank.sync()
    assert have == narrow and done == frames and len(batches) >= 3 and bank.total_frames == frames
    assert chan.total_samples == narrow * d1 * d2 and fine.total_samples == narrow * d2
    assert bits_equal(mid.cpu().numpy(), one), "stage one"
    assert bits_equal(out.cpu().numpy(), two), "the narrow streams"
    text = [[""], [""]]
    n_peaks = 0
    for a, z in batches:
        res = bank.poll(wait=True)
        n_peaks += check_batch_polled(res, outs, a, z, 1, text, 2)[1]
    assert bank.poll() is None
    assert n_peaks > 0 and sum(len(o["peak_frames"]) for o in outs) >= 6  # at least three cumulations per band
    for b, call in enumerate(e["calls"]):
        assert text[b][0] == decs[b][0][0] and call in text[b][0], text[b][0]
    for obj in (chan, fine, bank):
        obj.close()
    return skipped


def test_end_to_end_with_a_bank_on_one_stream(capi, e2e):
    """Every triple makes a whole number of hops."""
    assert chain(capi, e2e) == 0


def test_end_to_end_with_ragged_calls(capi, e2e):
    """The same stream cut as a receiver cuts it (ragged_lengths): the same samples, peaks, edges and text."""
    lens = ragged_lengths(e2e[1], F.E2E["hop"])
    assert len(lens) >= 8
    assert chain(capi, e2e, lens) >= 2  # (triples in which the bank was skipped)
