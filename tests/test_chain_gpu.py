"""The receive chain on the GPU (sdr_chain_*, csrc/capi_chain.hip): an endless ragged stream through a small ring gives the
oracle's bits.  Every case drives one raw cu8 stream through a chain in pushes drawn with a fixed seed and compares
  - the narrow streams, stitched from sdr_chain_read_narrow after every push, with the NumPy reference streams, bit for bit;
  - every polled batch with the oracle receiver fed those reference streams (parity_tools.check_batch_polled: peaks, edges,
    runes, frame indices), and the decoded text;
  - the batches each push enqueues (how many, first frame, frames) and the chain's counters with tests/chain_ref.py's plan.
The shapes are the existing end-to-end fixtures (2 bands, N = 512, hop 128, 1800 frames, cu8; the blanker's 1 band, 1460
frames): the smallest at which cuts, carries and wraps all occur hundreds of times.

Reading after every push constrains the lengths: a push of several pieces may move the ring's carry between two of its own
pieces, and what the first of them produced is then gone before the push returns.  ragged_pushes asks the plan (chain_ref, not
the library) and replaces such a length by one of at most a piece, which never does that."""
import copy
import ctypes as C

import numpy as np
import pytest

import chain_ref as CR
import ddc_ref as R
import fine_ref as F
import nb_ref as N
from parity_tools import bits_equal, capi, check_batch_polled, decode, frames_of, run_oracle  # noqa: F401
from sdrainer_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table(capi):
    return capi.ddc_nco_table()


# -- push lengths -------------------------------------------------------------------------------------------------------------
def ragged_pushes(plan_args, total, seed, lead=()):
    """Host push lengths as a USB stack delivers them, drawn with a fixed seed: one sample, fewer than a granule, more than a
    piece, odd ones between; `lead` in front.  They sum to `total`."""
    plan = CR.Plan(**plan_args)
    rng = np.random.default_rng(seed)
    lens = []
    for n in lead:
        plan.push(n, True)
        lens.append(n)
    left = total - sum(lens)
    while left:
        r = rng.random()
        if r < 0.1:
            n = 1
        elif r < 0.3:
            n = int(rng.integers(1, plan.g))
        elif r < 0.5:
            n = int(rng.integers(plan.piece + 1, plan.max_in + 1))
        else:
            n = 2 * int(rng.integers(plan.g // 2, plan.piece // 2)) + 1
        n = min(n, left)
        trial = copy.copy(plan)
        trial.push(n, True)
        if trial.base > plan.have:  # the push would drop samples of its own before they can be read (see above)
            n = min(int(rng.integers(plan.g, plan.piece + 1)), left)
        plan.push(n, True)
        lens.append(n)
        left -= n
    assert sum(lens) == total and max(lens) <= plan.max_in
    return lens


def granule_pushes(plan_args, total, seed):
    """Device push lengths: whole granules, from one granule to the capacity."""
    g, most = CR.granule(plan_args["total_decimation"], plan_args["nb_block"]), plan_args["max_in"]
    assert total % g == 0
    rng = np.random.default_rng(seed)
    lens, left = [g], total - g
    while left:
        lens.append(min(g * int(rng.integers(1, most // g + 1)), left))
        left -= lens[-1]
    return lens


# -- the driver ---------------------------------------------------------------------------------------------------------------
def drive(chain, bank, plan, raw, lens, ref, outs, text, host=True, wide_dev=None, pos=0, read_to=0):
    """Pushes raw[pos : pos + sum(lens)] in pieces of `lens`; after every push the counters and the batches against the plan,
    the new narrow samples read and every batch polled against the oracle.  Returns (pos, read_to, peaks delivered) and
    asserts the stitched narrow streams against ref [bands, samples, 2]."""
    n_bands = ref.shape[0]
    first, got, n_peaks = read_to, [[] for _ in range(n_bands)], 0
    sample_bytes = raw.dtype.itemsize * (raw.shape[1] if raw.ndim == 2 else 1)
    for n in lens:
        want = CR.batches_of(plan, n, host)
        if host:
            n_batches = chain.push_host(raw[pos:pos + n])
        else:
            n_batches = chain.push_device(wide_dev.data_ptr() + pos * sample_bytes, n)
        pos += n
        st = chain.stats()
        assert n_batches == len(want), (n, n_batches, want)
        assert (st["accepted"], st["processed"], st["pending"], st["resident_from"], st["narrow"], st["frames"], st["batches"],
                st["carry_moves"]) == plan.state(), (st, plan.state())
        assert st["processed"] + st["pending"] == st["accepted"] == pos
        if st["narrow"] > read_to:
            assert st["resident_from"] <= read_to
            for b in range(n_bands):
                got[b].append(chain.read_narrow(b, read_to, st["narrow"] - read_to))
            read_to = st["narrow"]
        for a, f in want:
            res = bank.poll(wait=True)
            assert res is not None, "a batch the plan predicts was not delivered"
            n_peaks += check_batch_polled(res, outs, a, a + f, 1, text, n_bands)[1]
    chain.sync()
    assert bank.poll() is None, "a batch the plan does not predict was delivered"
    if read_to > first:
        narrow = np.stack([np.concatenate(g) for g in got])
        assert bits_equal(narrow, np.ascontiguousarray(ref[:, first:read_to])), "the narrow streams"
    return pos, read_to, n_peaks


def check_geometry(chain, plan):
    st = chain.stats()
    assert (st["granule"], st["piece"], st["ring_samples"]) == (plan.g, plan.piece, plan.ring), (st, plan.g, plan.piece, plan.ring)
    assert st["reserved"] == 0 and st["accepted"] == 0


# -- channelizer + fine converter (fine_ref.E2E) -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fine_e2e(table):
    """The fixture through the reference chain and the oracle receiver, once for both cases."""
    e = F.E2E
    raw, narrow, one, two = F.e2e_reference(*table)
    centers = [14_000_000 + int(round(t * e["wide_rate"] / (F.L * e["d1"]))) for t in e["targets"]]
    _, outs, decs = run_oracle(e["rate"], e["n"], e["edge"], [[b] for b in e["bins"]], list(two), centers, e["hop"])
    return raw, narrow, two, centers, outs, decs


class FineRig:
    """Channelizer (M = 8, D = 4), fine converter (D = 8) and bank (N = 512, hop 128, 7 frames per batch at the most) in a
    chain.  The members' capacities are no multiples of the granule (64): piece = 33216 wide samples = 1038 narrow ones."""
    CHAN_MAX, FINE_MAX, MAX_BATCH = 33260, 8400, 7

    def __init__(self, capi, centers, max_in, ring):
        import torch

        e = F.E2E
        h1, h2 = F.e2e_taps()
        self.stream = torch.cuda.Stream()
        self.bank = capi.Bank(e["rate"], e["n"], n_bands=2, edge_width=e["edge"], max_batch_frames=self.MAX_BATCH, max_listeners=2, hop=e["hop"])
        self.chan = capi.Chan(e["n_channels"], e["d1"], h1, list(e["channels"]), in_format=capi.DDC_CU8, max_in_samples=self.CHAN_MAX)
        self.fine = capi.Fine(2, e["d2"], h2, list(e["fine_steps"]), max_in_samples=self.FINE_MAX)
        for b in range(2):
            self.bank.set_center_frequency(b, centers[b])
            assert self.bank.attach(b, e["bins"][b]) == 0
        self.bank.enable_results(True)
        # the chain is created on the null stream its members share and moved, members and all, by one call
        self.chain = capi.Chain(self.bank, chan=self.chan, fine=self.fine, max_in_samples=max_in, ring_samples=ring)
        self.chain.set_stream(self.stream.cuda_stream)
        self.plan_args = dict(total_decimation=e["d1"] * e["d2"], nb_block=1, limit=min(self.CHAN_MAX, self.FINE_MAX * e["d1"]),
                              block_size=e["n"], hop=e["hop"], max_batch_frames=self.MAX_BATCH, max_in=max_in, ring=ring)

    def close(self):
        self.chain.close()
        for o in (self.chan, self.fine, self.bank):
            o.close()


def check_texts(text, decs, calls):
    for b, call in enumerate(calls):
        assert text[b][0] == decs[b][0][0] and call in text[b][0], text[b][0]


def test_channelizer_fine_bank_host_pushes_through_the_minimum_ring(capi, fine_e2e):
    """Ragged host pushes - odd lengths, one sample, fewer than a granule, more than a piece - through the minimum ring: the
    carry moves at almost every piece, and a push of more than 896 narrow samples enqueues two batches of at most 7 frames."""
    e = F.E2E
    raw, narrow, two, centers, outs, decs = fine_e2e
    rig = FineRig(capi, centers, max_in=33216 + 5000, ring=0)
    plan = CR.Plan(**rig.plan_args)
    assert (plan.g, plan.piece, plan.ring) == (64, 33216, 2064)
    check_geometry(rig.chain, plan)
    lens = ragged_pushes(rig.plan_args, len(raw), seed=20_250)
    assert 1 in lens and any(1 < n < plan.g for n in lens) and sum(n > plan.piece for n in lens) >= 5 and sum(n % 2 for n in lens) >= 50
    text = [[""], [""]]
    pos, read_to, n_peaks = drive(rig.chain, rig.bank, plan, raw, lens, two, outs, text)
    st = rig.chain.stats()
    assert pos == len(raw) and read_to == narrow == st["narrow"] and st["pending"] == 0 and st["frames"] == e["frames"]
    assert st["carry_moves"] >= 10 and st["batches"] > e["frames"] // 7
    assert rig.bank.total_frames == e["frames"] and rig.chan.total_samples == len(raw) and rig.fine.total_samples == narrow * e["d2"]
    assert n_peaks > 0
    check_texts(text, decs, e["calls"])
    rig.close()


def test_channelizer_fine_bank_device_pushes_in_place(capi, fine_e2e):
    """The same chain fed from device memory in whole granules, the ring longer than the stream: nothing ever moves, and the
    narrow bits and the results are those of the host pushes (both are the reference's)."""
    import torch

    e = F.E2E
    raw, narrow, two, centers, outs, decs = fine_e2e
    rig = FineRig(capi, centers, max_in=40_000, ring=narrow + 8)
    plan = CR.Plan(**rig.plan_args)
    check_geometry(rig.chain, plan)
    with torch.cuda.stream(rig.stream):
        wide = torch.from_numpy(raw.copy()).cuda()  # (the shared fixture is read-only)
    rig.stream.synchronize()
    lens = granule_pushes(rig.plan_args, len(raw), seed=20_251)
    assert lens[0] == plan.g and max(lens) > plan.piece and len(lens) >= 100
    text = [[""], [""]]
    pos, read_to, n_peaks = drive(rig.chain, rig.bank, plan, raw, lens, two, outs, text, host=False, wide_dev=wide)
    st = rig.chain.stats()
    assert pos == len(raw) and read_to == narrow and st["carry_moves"] == 0 and st["resident_from"] == 0 and st["frames"] == e["frames"]
    assert bits_equal(np.stack([rig.chain.read_narrow(b, 0, narrow) for b in range(2)]), two)  # (still resident, all of it)
    assert n_peaks > 0
    check_texts(text, decs, e["calls"])
    rig.close()


# -- down-converter alone (ddc_ref.E2E), overlapped and dense frames ----------------------------------------------------------
@pytest.fixture(scope="module")
def ddc_e2e(table):
    e = R.E2E
    raw, narrow = R.e2e_wide()
    ref = R.ddc_ref(R.to_f32(raw, R.CU8), e["decimation"], R.e2e_taps(), e["steps"], *table)
    centers = [14_000_000 + int(round(s * e["wide_rate"] / R.L)) for s in e["steps"]]
    for a in (raw, ref):
        a.setflags(write=False)
    return raw, narrow, ref, centers


@pytest.fixture(scope="module")
def ddc_oracle(ddc_e2e):
    """hop -> (oracle outputs, text per band): hop 128 as everywhere, and dense frames (the bank's hop = 0)."""
    e = R.E2E
    raw, narrow, ref, centers = ddc_e2e
    out = {}
    for hop in (e["hop"], e["n"]):
        bins = [[b] for b in e["bins"]]
        if hop == e["n"]:
            _, outs, _ = run_oracle(e["rate"], e["n"], e["edge"], bins, [frames_of(s, e["n"], hop) for s in ref], centers)
            texts = [decode(o["deb"][:, 0], e["rate"], hop)[0] for o in outs]
        else:
            _, outs, decs = run_oracle(e["rate"], e["n"], e["edge"], bins, list(ref), centers, hop)
            texts = [d[0][0] for d in decs]
        out[hop] = (outs, texts)
    return out


class DdcRig:
    """Down-converter (D = 8, two bands) and bank in a chain, optionally behind a blanker: granule 16 (the blanker's block
    with one), piece 8992 wide samples = 1124 narrow ones."""
    DDC_MAX = 9000

    def __init__(self, capi, e, centers, hop, max_in, ring=0, max_batch=64, nb=None, taps=None, ddc_max=None):
        import torch

        self.stream = torch.cuda.Stream()
        n_bands = len(e["steps"])
        self.bank = capi.Bank(e["rate"], e["n"], n_bands=n_bands, edge_width=e["edge"], max_batch_frames=max_batch, max_listeners=2, hop=hop)
        self.ddc = capi.Ddc(e["decimation"], R.e2e_taps() if taps is None else taps, e["steps"], in_format=capi.DDC_CU8,
                            max_in_samples=ddc_max or self.DDC_MAX)
        self.nb = nb
        for o in (self.bank, self.ddc) + ((nb,) if nb else ()):
            o.set_stream(self.stream.cuda_stream)
        for b in range(n_bands):
            self.bank.set_center_frequency(b, centers[b])
            assert self.bank.attach(b, e["bins"][b]) == 0
        self.bank.enable_results(True)
        self.chain = capi.Chain(self.bank, ddc=self.ddc, nb=nb, max_in_samples=max_in, ring_samples=ring)
        limit = min(ddc_max or self.DDC_MAX, nb.cfg.max_in_samples if nb else 1 << 30)
        self.plan_args = dict(total_decimation=e["decimation"], nb_block=nb.block if nb else 1, limit=limit, block_size=e["n"],
                              hop=hop or e["n"], max_batch_frames=max_batch, max_in=max_in, ring=ring)

    def close(self):
        self.chain.close()
        for o in (self.ddc, self.bank) + ((self.nb,) if self.nb else ()):
            o.close()


@pytest.mark.parametrize("hop", [128, 0], ids=["hop128", "dense"])
def test_ddc_bank_overlapped_and_dense_frames(capi, ddc_e2e, ddc_oracle, hop):
    """No blanker, no fine converter: stage one writes straight into the ring.  With dense frames (hop = 0: block_size) a
    batch leaves no history, and twelve pushes of exactly one frame in front make the carry move with nothing to move."""
    e = R.E2E
    raw, narrow, ref, centers = ddc_e2e
    eff = hop or e["n"]
    outs, texts = ddc_oracle[eff]
    rig = DdcRig(capi, e, centers, hop, max_in=8992 + 3000)
    plan = CR.Plan(**rig.plan_args)
    assert (plan.g, plan.piece, plan.ring) == (16, 8992, 2148)
    check_geometry(rig.chain, plan)
    lead = [e["n"] * e["decimation"]] * 12 if hop == 0 else []
    lens = ragged_pushes(rig.plan_args, len(raw), seed=20_252 + hop, lead=lead)
    trial = CR.Plan(**rig.plan_args)
    moved = [a for n in lens for a in trial.push(n, True) if a[0] == "move"]
    assert len(moved) >= 10 and (hop != 0 or any(a[3] == 0 for a in moved)), "the carry never moved empty"
    text = [[""], [""]]
    pos, read_to, n_peaks = drive(rig.chain, rig.bank, plan, raw, lens, ref, outs, text)
    st = rig.chain.stats()
    frames = (narrow - e["n"]) // eff + 1
    assert pos == len(raw) and read_to == narrow and st["frames"] == frames == rig.bank.total_frames and st["carry_moves"] == len(moved)
    assert n_peaks > 0 and [t[0] for t in text] == texts
    if hop:
        assert all(call in t for call, t in zip(e["calls"], texts))
    rig.close()


# -- blanker + down-converter -------------------------------------------------------------------------------------------------
NB_CHAIN = dict(R.E2E, steps=(9000,), bins=(320,), texts=("dl1abc dl1abc",), calls=("dl1abc",), dit_ticks=(8,), frames=1460, sigma=0.1,
                pulses=300, block=256, window=8, hold=3, ratio=192)


def nb_chain_wide():
    """One keyed carrier and noise as ddc_ref's fixture builds them, cu8, with samples (255, 0) planted at random places
    behind the blanker's warm-up (what tests/test_nb_gpu.py's chain feeds)."""
    e = NB_CHAIN
    narrow = (e["frames"] - 1) * e["hop"] + e["n"]
    wide = narrow * e["decimation"]
    offset = e["steps"][0] * e["wide_rate"] / R.L + (e["bins"][0] - e["n"] // 2) * e["rate"] / e["n"]
    key = np.repeat(np.concatenate([np.zeros(40, np.uint8), synth.keying_pattern(e["texts"][0], e["dit_ticks"][0])]), e["hop"] * e["decimation"])
    raw = synth.wide_stream(wide, e["wide_rate"], [(offset, e["amplitude"], key)], noise_sigma=e["sigma"], seed=e["seed"], quantise="cu8")
    places = np.sort(np.random.default_rng(5).choice(np.arange(e["window"] * e["block"], wide), e["pulses"], replace=False))
    raw[places] = (255, 0)
    return raw, narrow


def test_blanker_ddc_bank(capi, table):
    """nb_ref, then ddc_ref, then the oracle.  The blanker's block, 256, does not divide 2 * D = 16: the granule is the lcm,
    256, and a piece is 39 blocks (the down-converter's capacity, 10000, is no multiple of either)."""
    e = NB_CHAIN
    raw, narrow = nb_chain_wide()
    blanked, stats = N.nb_ref(raw, N.CU8, e["block"], e["window"], e["ratio"], e["hold"])
    assert stats["impulses"] >= e["pulses"] // 2 and not np.array_equal(blanked, raw)
    ref = R.ddc_ref(R.to_f32(blanked, R.CU8), e["decimation"], R.e2e_taps(), e["steps"], *table)
    centers = [14_000_000 + int(round(e["steps"][0] * e["wide_rate"] / R.L))]
    _, outs, decs = run_oracle(e["rate"], e["n"], e["edge"], [[e["bins"][0]]], list(ref), centers, e["hop"])
    nb = capi.Nb(capi.DDC_CU8, e["block"], e["window"], e["ratio"], e["hold"], max_in_samples=40 * e["block"])
    rig = DdcRig(capi, e, centers, e["hop"], max_in=9984 + 3000, nb=nb, ddc_max=10_000)
    plan = CR.Plan(**rig.plan_args)
    assert (plan.g, plan.piece, plan.ring) == (256, 9984, 2272) and plan.g not in (2 * e["decimation"], 16)
    check_geometry(rig.chain, plan)
    lens = ragged_pushes(rig.plan_args, len(raw), seed=20_254)
    text = [[""]]
    pos, read_to, n_peaks = drive(rig.chain, rig.bank, plan, raw, lens, ref, outs, text)
    st = rig.chain.stats()
    assert pos == len(raw) and read_to == narrow and st["frames"] == e["frames"] and st["carry_moves"] >= 10 and st["pending"] == 0
    assert nb.read_stats() == stats and nb.total_samples == len(raw)
    assert n_peaks > 0
    check_texts(text, decs, e["calls"])
    rig.close()


# -- statuses -----------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(capi, ddc_e2e, ddc_oracle):
    """Every create refusal one GPU can produce, then every push and read refusal between good pushes of the down-converter's
    chain: the stream goes on bit-exact behind each.  Last, a member driven directly: the push behind it is refused, the
    chain is destroyed, and the members go on by hand from where the direct call left them."""
    import torch

    L = capi.load()
    vp = C.c_void_p
    e = R.E2E
    raw, narrow, ref, centers = ddc_e2e
    outs, _ = ddc_oracle[e["hop"]]
    rig = DdcRig(capi, e, centers, e["hop"], max_in=8992 + 3000)
    bank, ddc, stream = rig.bank, rig.ddc, rig.stream.cuda_stream
    taps = R.e2e_taps()

    def on_stream(o):
        o.set_stream(stream)
        return o

    # members that do not fit: another format, another stream count, another band count, another stream, too small a capacity
    nb_cs8 = on_stream(capi.Nb(capi.DDC_CS8, 256, 8, 192, 3, max_in_samples=4096))
    fine3 = on_stream(capi.Fine(3, 8, taps, [0, 0]))
    chan = on_stream(capi.Chan(8, 4, F.e2e_taps()[0], [1, 6], in_format=capi.DDC_CU8))
    bank1 = on_stream(capi.Bank(e["rate"], e["n"], n_bands=1, edge_width=e["edge"], max_batch_frames=64, max_listeners=2, hop=e["hop"]))
    ddc_null = capi.Ddc(e["decimation"], taps, e["steps"], in_format=capi.DDC_CU8, max_in_samples=9000)  # stays on the null stream
    ddc_tiny = on_stream(capi.Ddc(e["decimation"], taps, e["steps"], in_format=capi.DDC_CU8, max_in_samples=8))
    # banks in a state a chain refuses
    dense = dict(n_bands=2, edge_width=e["edge"], max_batch_frames=64, max_listeners=2)
    bank_graph = on_stream(capi.Bank(e["rate"], e["n"], **dense))
    bank_graph.graph_capture(4)
    bank_staged = on_stream(capi.Bank(e["rate"], e["n"], hop=e["hop"], **dense))
    assert bank_staged.push_iq(0, e["rate"], np.zeros((e["hop"], 2), np.float32)) == capi.OK
    bank_defer = on_stream(capi.Bank(e["rate"], e["n"], hop=e["hop"], **dense))
    bank_defer.enable_results(True)
    bank_defer.defer_listen(True)

    def config(**kw):
        c = capi.ChainConfig(C.sizeof(capi.ChainConfig), 11_992, 0, 0, None, ddc._h, None, None, bank._h)
        for k, v in kw.items():
            setattr(c, k, v._h if hasattr(v, "_h") else v)
        return c

    h = vp()
    create = L.sdr_chain_create
    refusals = [
        (capi.ERR_BAD_ARG, create, None, C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config()), None),
        (capi.ERR_BAD_ARG, create, C.byref(config(struct_size=48)), C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config(reserved=1)), C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config(max_in_samples=0)), C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config(bank=None)), C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config(chan=chan)), C.byref(h)),            # both stage ones
        (capi.ERR_BAD_ARG, create, C.byref(config(ddc=None)), C.byref(h)),             # neither
        (capi.ERR_BAD_ARG, create, C.byref(config(nb=nb_cs8)), C.byref(h)),            # cs8 in front of cu8
        (capi.ERR_BAD_ARG, create, C.byref(config(fine=fine3)), C.byref(h)),           # three inputs behind two bands
        (capi.ERR_BAD_ARG, create, C.byref(config(bank=bank1)), C.byref(h)),           # two bands into a bank of one
        (capi.ERR_BAD_ARG, create, C.byref(config(ddc=ddc_null)), C.byref(h)),         # members on different streams
        (capi.ERR_BAD_ARG, create, C.byref(config(ddc=ddc_tiny)), C.byref(h)),         # piece < G: not one granule of 16 fits 8
        (capi.ERR_BAD_ARG, create, C.byref(config(ring_samples=2144)), C.byref(h)),    # below the minimum, 2148
        (capi.ERR_BAD_ARG, create, C.byref(config(ring_samples=2150)), C.byref(h)),    # no multiple of 4
        (capi.ERR_STATE, create, C.byref(config(bank=bank_graph)), C.byref(h)),
        (capi.ERR_STATE, create, C.byref(config(bank=bank_staged)), C.byref(h)),
        (capi.ERR_STATE, create, C.byref(config(bank=bank_defer)), C.byref(h)),
    ]
    for status, call, *args in refusals:
        h.value = 0xdead
        assert call(*args) == status, (args, L.sdr_last_error())
        assert h.value == 0xdead and L.sdr_last_error()
    assert L.sdr_chain_destroy(None) == capi.OK

    chain, plan = rig.chain, CR.Plan(**rig.plan_args)
    g = plan.g
    with torch.cuda.stream(rig.stream):
        wide = torch.from_numpy(raw[:1 << 18].copy()).cuda()
    rig.stream.synchronize()
    n_b = C.c_int(-5)
    out4 = np.zeros(8, np.float32)
    fp = out4.ctypes.data_as(C.POINTER(C.c_float))
    host = vp(raw.ctypes.data)
    # (what, expected status, call, arguments...); the chain has nothing pending where the list starts
    push_refusals = [
        ("device length no multiple of G", capi.ERR_BAD_SIZE, L.sdr_chain_push_device, chain._h, vp(wide.data_ptr()), g * 5 + 8, C.byref(n_b)),
        ("device pointer misaligned", capi.ERR_BAD_ARG, L.sdr_chain_push_device, chain._h, vp(wide.data_ptr() + 8), g * 5, C.byref(n_b)),
        ("device null", capi.ERR_BAD_ARG, L.sdr_chain_push_device, chain._h, None, g * 5, C.byref(n_b)),
        ("host zero samples", capi.ERR_BAD_SIZE, L.sdr_chain_push_host, chain._h, host, 0, C.byref(n_b)),
        ("host above the capacity", capi.ERR_BAD_SIZE, L.sdr_chain_push_host, chain._h, host, 11_993, C.byref(n_b)),
        ("device zero samples", capi.ERR_BAD_SIZE, L.sdr_chain_push_device, chain._h, vp(wide.data_ptr()), 0, C.byref(n_b)),
        ("device above the capacity", capi.ERR_BAD_SIZE, L.sdr_chain_push_device, chain._h, vp(wide.data_ptr()), 12_000, C.byref(n_b)),
        ("host null", capi.ERR_BAD_ARG, L.sdr_chain_push_host, chain._h, None, 100, C.byref(n_b)),
        ("read in front of the resident range", capi.ERR_BAD_ARG, L.sdr_chain_read_narrow, chain._h, 0, -1, 4, fp),
        ("read behind the resident range", capi.ERR_BAD_ARG, L.sdr_chain_read_narrow, chain._h, 0, 0, 1 << 20, fp),
        ("read nothing", capi.ERR_BAD_ARG, L.sdr_chain_read_narrow, chain._h, 0, 0, 0, fp),
        ("read band 2 of 2", capi.ERR_BAD_ARG, L.sdr_chain_read_narrow, chain._h, 2, 0, 4, fp),
        ("read to null", capi.ERR_BAD_ARG, L.sdr_chain_read_narrow, chain._h, 0, 0, 4, None),
        ("stats to null", capi.ERR_BAD_ARG, L.sdr_chain_stats, chain._h, None),
    ]
    text = [[""], [""]]
    pos = read_to = 0
    rng = np.random.default_rng(20_255)
    for what, status, call, *args in [(None, None, None)] + push_refusals:
        if call:
            before = chain.stats()
            assert call(*args) == status, (what, L.sdr_last_error())
            assert n_b.value == -5 and L.sdr_last_error() and chain.stats() == before, what
        # a good device push of whole granules (nothing is pending), then a good ragged host push that leaves samples pending
        # and its remainder, so that the next refusal again finds nothing pending
        k = g * int(rng.integers(1, 600))
        pos, read_to, _ = drive(chain, bank, plan, raw, [k], ref, outs, text, host=False, wide_dev=wide, pos=pos, read_to=read_to)
        odd = 2 * int(rng.integers(8, 3000)) + 1
        pos, read_to, _ = drive(chain, bank, plan, raw, [odd], ref, outs, text, pos=pos, read_to=read_to)
        assert chain.stats()["pending"] == odd % g != 0
        assert L.sdr_chain_push_device(chain._h, vp(wide.data_ptr()), g, C.byref(n_b)) == capi.ERR_STATE, "a device push with samples pending"
        assert n_b.value == -5 and chain.stats()["accepted"] == pos
        pos, read_to, _ = drive(chain, bank, plan, raw, [g - chain.stats()["pending"]], ref, outs, text, pos=pos, read_to=read_to)
        assert chain.stats()["pending"] == 0
    assert read_to > 20 * e["n"] and chain.stats()["carry_moves"] >= 3 and pos + 4 * g < wide.shape[0]
    # the next read range is the resident one exactly: its two ends are readable, one sample further on either side is not
    st = chain.stats()
    assert bits_equal(chain.read_narrow(1, st["resident_from"], 1)[0], ref[1, st["resident_from"]])
    assert L.sdr_chain_read_narrow(chain._h, 1, st["resident_from"] - 1, 1, fp) == capi.ERR_BAD_ARG
    assert L.sdr_chain_read_narrow(chain._h, 1, st["narrow"], 1, fp) == capi.ERR_BAD_ARG

    # a member driven directly: the down-converter takes the stream's next 64 wide samples by hand
    d = e["decimation"]
    side = torch.zeros((2, 16, 2), dtype=torch.float32, device="cuda")
    ddc.process_device(wide.data_ptr() + pos * 2, 8 * d, side.data_ptr(), 16)
    ddc.sync()
    assert bits_equal(side.cpu().numpy()[:, :8], ref[:, read_to:read_to + 8]), "the direct call continues the stream"
    before = chain.stats()
    assert L.sdr_chain_push_host(chain._h, vp(raw.ctypes.data + 2 * pos), 100, C.byref(n_b)) == capi.ERR_STATE and n_b.value == -5
    assert L.sdr_chain_push_device(chain._h, vp(wide.data_ptr() + pos * 2), g, C.byref(n_b)) == capi.ERR_STATE
    assert chain.stats() == before and ddc.total_samples == pos + 8 * d and bank.total_frames == before["frames"]
    # destroying the chain leaves the members usable: one more call by hand, against the reference
    chain.close()
    ddc.process_device(wide.data_ptr() + (pos + 8 * d) * 2, 8 * d, side.data_ptr() + 8 * 8, 16)
    ddc.sync()
    assert bits_equal(side.cpu().numpy(), ref[:, read_to:read_to + 16]), "the down-converter by hand behind the chain"
    # and the bank: its next frames from a buffer of the reference's samples, against the oracle
    done = before["frames"]
    span = torch.from_numpy(np.ascontiguousarray(ref[:, done * e["hop"]:done * e["hop"] + 4 * e["hop"] + e["n"]])).cuda()
    torch.cuda.synchronize()
    bank.process_device_stream(span.data_ptr(), 5, span.shape[1])
    res = bank.poll(wait=True)
    check_batch_polled(res, outs, done, done + 5, 1, text, 2)
    assert bank.total_frames == done + 5
    for o in (nb_cs8, fine3, chan, bank1, ddc_null, ddc_tiny, bank_staged, bank_defer):
        o.close()
    bank_graph.graph_release()
    bank_graph.close()
    rig.close()
