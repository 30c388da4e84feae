"""The peak scan at word, span and row ends and at its capacities, bit for bit against the oracle (the inputs:
tests/peak_shape_gen.py; what makes each case what its name says: tests/test_peak_shape_host.py).

k_find_peaks / k_find_peaks_wide find runs by bit operations on 64-bin flag words, k_cum_refine lists candidates per span
of 4096 bins (16384 in the wide shape) and reaches the bin beside a word or span end only through its halo terms; the
carriers of the other tests sit 8 bins apart inside the edges.  Here, with the word end w = 64 and the span ends S = 4096
(also 8192 and 12288 at N = 16384, and 16384 at N = 32768), at N = 512, 8192 (k_find_peaks, two narrow spans), 16384 (the
largest row held in LDS) and 32768 (k_find_peaks_wide):

  case a   (0, 2) max 0 (y1 = 0) | (w-2, w+1) max w | (2w-1) and (4w) single | (310, 450): two whole words |
           (n-7, n-1) max n-1 (open run, y3 = 0) | (S-2, S+1) max S-1
  case b   (0) and (n-1) single | (63) and (65) single, one clear bin between | (2w-2, 2w+1) max 2w-1 | (3w-1) and (5w) single |
           (S-2, S+1) max S.  The maximum on a word's last bit sits at the SECOND word's end (2w-1, not w-1): 63 and 65 hold
           the first word's end, and a run start's `flags[w - 1] >> 63` is the same code at every word
  case c   (n-230, n-1) max n-230: one open run from mid-word over three words and more | (S-1) single
  case d   (0, 2) max 2 | (n-7, n-1) max n-7 | (S) single                                             (N >= 8192)
  tied     shifted_tied, shift 3, peak threshold 1 dB: exactly tied pairs (4k+3, 4k+4) across every word and span end,
           the first bin reported, and single-bin runs at 0 and N - 1                                  (N = 512, 8192)

two or three uneven batches each; case a and the tied case also with the cuts 99, 1, 98, 2, 97, 3, 100 (cumulations whose
first slot holds 1, 2 and 3 frames - the refinement's four lanes per column find cnt <= 0 - and a batch that is exactly
one cumulation); one N = 512 row through hipGraph replays and one through the staging buffers; one row of two bands with
a different case each.  The listener row (N = 16384) puts listeners on 0, N - 1, 4095 | 4096 | 4097 (tap entries that
overlap and cross a span), 8191, a single-bin carrier at 12288 and the first bin of a six-bin run: under
tests/test_forced_paths.py's SDR_FFT_R32 rows the refinement reads those columns from the wide tap, the others of the same
run from the psd array.  By default these short batches take Refine::NONE: tests/test_forced_paths.py runs this module
with the bound-and-refine path forced, in both refinement shapes.

Capacities: more runs than max_peaks (129 tied runs on banks of 1, 64 and 129 - the exact fit; nine runs on a bank of 4,
followed in the stream and in one batch by cumulations of two): the first max_peaks peaks are delivered, peaks_found and
sdr_read_peaks' *n_out say how many there were, first_peak follows on, sdr_poll's SDR_ERR_BAD_SIZE asks for what is
stored; the same through a group.  More edges than a batch stores (8192): the first 8192 are delivered, the rest counted
in edges_dropped, and the decoder - which reads the edge positions, not the stored records - saw every one."""
import ctypes as C

import numpy as np
import pytest

import peak_shape_gen as gen
from oracle import oracle as orc
from parity_case import Case
from parity_tools import GROUP_CENTER, Pair, capi, check_batch_polled, transitions  # noqa: F401 (capi: the fixture)
from sdrainer_amd import synth

pytestmark = pytest.mark.gpu


def make_case(row, cls=Case):
    bands = [(b.iq(), None, []) for b in row.bands]
    case = cls(row.n, len(bands), None, 0, [("batch", x) for x in row.batches], seed=0, rate=gen.RATES[row.n], path=row.path, bands=bands,
               init_bins=row.listeners, max_peaks=row.max_peaks, threshold=[b.threshold for b in row.bands])
    case.run_oracle()
    for b, band in enumerate(row.bands):  # the oracle this run compares with holds the designed runs (frequencies and values are its own)
        got = [[(p[0], p[1], p[6]) for p in pk] for pk in case.outs[b]["peaks"]]
        assert got == [band.expected(c) for c in range(row.cumulations)], f"{row.id} band {b}: not the designed runs"
    return case


@pytest.mark.parametrize("row", gen.GEOMETRY + gen.LISTENERS, ids=lambda r: r.id)
def test_peak_geometry(capi, row):
    case = make_case(row)
    case.run(capi, min_edges=0, activity=False).close()
    assert case.peaks == sum(sum(row.counts(b)) for b in range(len(row.bands)))
    if row.listeners[0]:
        assert case.edges > 0  # (the listeners sit on carriers)


SENTINEL = -7


class CapacityCase(Case):
    """A Case on a bank whose max_peaks is below the runs of some cumulation.  On top of what every Case compares (the
    shared checks know the bank's max_peaks): every batch is first polled with a peaks buffer one record short of what the
    batch stores - SDR_ERR_BAD_SIZE, n_peaks = the stored count - and then with exactly that many; and sdr_read_peaks is
    called with every kind of `max`."""

    polled = sized = reads = 0

    def stored(self, a, e):
        return sum(min(len(out["peaks"][gc]), self.max_peaks) for out in self.outs for gc, f in enumerate(out["peak_frames"]) if a <= f < e)

    def new_bank(self, capi, stream=None):
        bank = super().new_bank(capi, stream)
        plain, case = bank.poll, self

        def poll(wait=False, copy=True):
            r, want = bank._res, case.stored(*case.spans[case.polled])
            cap = r.peaks_cap
            try:
                if want:
                    r.peaks_cap = want - 1
                    rc = bank._L.sdr_poll(bank._h, C.byref(r), 1)
                    assert rc == capi.ERR_BAD_SIZE and r.n_peaks == want, f"batch {case.polled}: status {rc}, {r.n_peaks} peaks asked for, {want} stored"
                    case.sized += 1
                r.peaks_cap = want
                res = plain(wait, copy)
            finally:
                r.peaks_cap = cap
            case.polled += 1
            return res

        bank.poll = poll
        self.capi = capi
        return bank

    def check_device(self, bank, a, e, k, cumulations=True):
        super().check_device(bank, a, e, k, cumulations)
        for b in range(self.n_bands):
            for c in range(bank.last_batch_chunks):
                for mx in sorted({0, 1, self.max_peaks - 1, self.max_peaks, self.max_peaks + 5}):
                    arr = (self.capi.Peak * (mx + 2))()
                    for p in arr:
                        p.from_ = SENTINEL
                    n, fr = C.c_int(-1), C.c_int(-1)
                    rc = bank._L.sdr_read_peaks(bank._h, b, c, arr, mx, C.byref(n), C.byref(fr))
                    assert rc == 0, bank._L.sdr_last_error().decode()
                    want = self.outs[b]["peaks"][list(self.outs[b]["peak_frames"]).index(a + fr.value)]
                    filled = min(len(want), self.max_peaks, mx)
                    assert n.value == len(want), f"band {b} chunk {c} max {mx}: *n_out {n.value}, the oracle found {len(want)}"
                    assert [arr[i].astuple() for i in range(filled)] == want[:filled], f"band {b} chunk {c} max {mx}"
                    assert all(arr[i].from_ == SENTINEL for i in range(filled, mx + 2)), f"band {b} chunk {c} max {mx}: written beyond {filled} records"
                    self.reads += 1


@pytest.mark.parametrize("row", gen.CAPACITY, ids=lambda r: r.id)
def test_peak_capacity(capi, row):
    case = make_case(row, CapacityCase)
    counts = row.counts()
    assert max(counts) >= row.max_peaks and (max(counts) > row.max_peaks) == (row.id != gen.EXACT_FIT)
    case.run(capi, min_edges=0, activity=False).close()
    assert case.peaks == sum(min(c, row.max_peaks) for c in counts)
    assert case.polled == len(row.batches) and case.sized >= 1 and case.reads > 0


def test_peak_capacity_through_a_group(capi):
    """One batch of three cumulations on two bands: nine runs and then two on a bank of max_peaks = 4, and 129 tied runs -
    through one bank and through a group of two members, which deliver the same."""
    row = gen.GROUP
    n, rate, frames, cap = row.n, gen.RATES[row.n], row.frames, row.max_peaks
    edge = synth.default_edge_width(n)
    iq = np.stack([b.iq() for b in row.bands])
    outs = []
    for b, band in enumerate(row.bands):
        r = orc.Receiver(rate, n, edge, band.threshold, 1, center_frequency=GROUP_CENTER[b])
        outs.append(r.process(iq[b]))
    found = [len(pk) for out in outs for pk in out["peaks"]]
    assert found == [9, 2, 2, 129, 129, 129]
    stored = sum(min(f, cap) for f in found)
    p = Pair(capi, (0, 0), rate, n, n_bands=2, edge_width=edge, max_listeners=1, max_batch_frames=frames, max_peaks=cap)
    for b, band in enumerate(row.bands):
        if band.threshold != 15.0:
            p.bank.set_peak_threshold(b, band.threshold)
            p.group.set_peak_threshold(b, band.threshold)
    p.bank.enable_results(True)
    p.group.enable_results(True)
    p.process(iq)
    for who, entry in ((p.bank, p.bank._L.sdr_poll), (p.group, p.group._L.sdr_group_poll)):
        r = who._res
        keep, r.peaks_cap = r.peaks_cap, stored - 1
        try:
            rc = entry(who._h, C.byref(r), 1)
        finally:
            r.peaks_cap = keep
        assert rc == capi.ERR_BAD_SIZE and r.n_peaks == stored, (rc, r.n_peaks, stored)
    res = p.polls()  # (the group's delivery equals the bank's, field by field)
    assert [int(x) for x in res["chunks"]["peaks_found"]] == found
    assert [int(x) for x in res["chunks"]["n_peaks"]] == [min(f, cap) for f in found]
    _, n_peaks = check_batch_polled(res, outs, 0, frames, None, [[], []], 2, live=[[], []], max_peaks=cap)
    assert n_peaks == stored == len(res["peaks"])
    assert p.polls(wait=False) is None
    assert p.group.read_drop_counters() == p.bank.read_drop_counters() == (0, 0)
    p.close()


# -- more edges than a batch stores -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_run():
    """The edge row's input and the oracle over the whole of it."""
    iq, b = gen.edge_stream()
    n = gen.EDGE_N
    ref = orc.Receiver(gen.EDGE_RATE, n, synth.default_edge_width(n), 15.0, 1)
    ref.attach(b)
    out = ref.process(iq)
    count = len(transitions(out["deb"][:, 0], 0, gen.EDGE_FRAMES)[0])
    assert count > gen.EDGE_CAP
    return iq, b, ref, out, count


def edge_bank(capi, b):
    bank = capi.Bank(gen.EDGE_RATE, gen.EDGE_N, max_batch_frames=gen.EDGE_FRAMES, max_listeners=1, signal_debounce=1)
    assert bank.attach(0, b) == 0
    return bank


def test_edge_capacity_read(capi, edge_run):
    iq, b, ref, out, count = edge_run
    F, cap, deb = gen.EDGE_FRAMES, gen.EDGE_CAP, out["deb"][:, 0]
    bank = edge_bank(capi, b)
    assert bank.process_host(iq[:F]) == F
    got = np.zeros(F, capi.EDGE_DTYPE)
    got["frame"], got["state"] = 0xffffffff, 0xffffffff
    n = C.c_int(-1)
    assert bank._L.sdr_read_edges(bank._h, 0, 0, C.c_void_p(got.ctypes.data), F, C.byref(n)) == 0
    trans, states = transitions(deb, 0, F)
    assert n.value == count == len(trans), f"*n_out {n.value}, the oracle has {count} edges"
    assert np.array_equal(got["frame"][:cap], trans[:cap]) and np.array_equal(got["state"][:cap], states[:cap]), "the first 8192 edges"
    assert np.all(got["frame"][cap:] == 0xffffffff) and np.all(got["state"][cap:] == 0xffffffff), "written beyond the 8192 edges a batch stores"
    assert bank.read_drop_counters() == (0, count - cap)
    assert np.array_equal(bank.read_keying_bits(0, 0), deb[:F])
    text = bank.read_text(0, 0)
    assert bank.process_host(iq[F:]) == gen.EDGE_TAIL
    trans, states = transitions(deb, F, F + gen.EDGE_TAIL)
    ed = bank.read_edges(0, 0)
    assert 0 < len(trans) < cap and np.array_equal(ed["frame"], trans) and np.array_equal(ed["state"], states), "the keyed batch's edges"
    assert np.array_equal(bank.read_keying_bits(0, 0), deb[F:])
    text += bank.read_text(0, 0)
    assert text == ref.text(0) and "dl1abc" in text, "the decoder did not see every edge"
    assert np.array_equal(bank.read_decoder_state(0, 0), ref.decoder_state(0))
    assert bank.read_drop_counters() == (0, count - cap)
    bank.close()


def test_edge_capacity_polled(capi, edge_run):
    iq, b, ref, out, count = edge_run
    F, cap = gen.EDGE_FRAMES, gen.EDGE_CAP
    bank = edge_bank(capi, b)
    bank.enable_results(True)
    assert bank.process_host(iq[:F]) == F
    res = bank.poll(wait=True)
    assert res["batch_index"] == 0 and res["first_frame"] == 0 and res["n_frames"] == F
    assert res["edges_dropped"] == count - cap and res["runes_dropped"] == 0
    assert len(res["listeners"]) == 1 and len(res["edges"]) == cap
    lr = res["listeners"][0]
    assert (lr["band"], lr["listener"], lr["first_edge"], lr["n_edges"], lr["first_rune"]) == (0, 0, 0, cap, 0)
    trans, states = transitions(out["deb"][:, 0], 0, F)
    assert np.array_equal(res["edges"]["frame"], trans[:cap]) and np.array_equal(res["edges"]["state"], states[:cap])
    text = [["".join(chr(int(x)) for x in res["runes"][:lr["n_runes"]])]]
    assert bank.process_host(iq[F:]) == gen.EDGE_TAIL
    res = bank.poll(wait=True)
    assert res["batch_index"] == 1
    # the next batch: its offsets start again at 0, its edges are the oracle's, the counter stays (since bank creation)
    n_edges, _ = check_batch_polled(res, [out], F, F + gen.EDGE_TAIL, 1, text, 1, edges_dropped=count - cap)
    assert 0 < n_edges == len(res["edges"]) and res["listeners"][0]["first_edge"] == 0
    assert text[0][0] == ref.text(0) and "dl1abc" in text[0][0], "the decoder did not see every edge"
    assert np.array_equal(bank.read_decoder_state(0, 0), ref.decoder_state(0))
    assert bank.read_drop_counters() == (0, count - cap)
    assert bank.poll(wait=False) is None
    bank.close()
