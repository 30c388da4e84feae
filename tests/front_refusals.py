"""The refusals of the front-end objects (sdr_ddc, sdr_chan, sdr_fine, sdr_nb and the sdr_chain that drives them) as one table:
what tests/test_front_refusals_gpu.py runs and compares, status and sdr_last_error() text, with tests/golden/front_refusals.json.

Every refusal the lists of test_{ddc,chan,fine,nb,iqc,chain}_gpu.py exercise is here at the smallest shapes, and one call that
is wrong in two ways per boundary between two checks (null before size, size before alignment, alignment before stride or
overlap, in-stride before out-stride), which pins the order of the checks.  No case's text contains a runtime's error string.

record() writes the golden file; it is no test.  It was run once, with the library as it stood before the objects got their
common core (csrc/front.h), from tests/:  python -m front_refusals"""
import ctypes as C
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "front_refusals.json")

vp = C.c_void_p
i32p = C.POINTER(C.c_int32)
fp = C.POINTER(C.c_float)

D, T, STEPS, CAP = 4, 8, (100, -200), 64   # stage one: decimation, taps, two bands, max_in_samples (cu8)
PIECE = 16                                 # a good call: 4 outputs per band
OUT_STRIDE = 16
FD, FT, FCAP = 2, 4, 64                    # the fine converter: two inputs, two bands
B, W = 64, 1                               # the blanker: block, window
NB_CAP = 4 * B
BANK_N, BANK_HOP, BANK_RATE = 512, 128, 48_000
CHAIN_MAX = 128                            # the chain's max_in_samples; its granule and piece are 64 = lcm(2 * 4 * 2, 64, 16)
G = 64
MIN_RING = 2 * BANK_N + G // (D * FD)      # 1032


def _taps(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32)


def _ints(keep, *v):
    a = np.array(v, np.int32)
    keep.append(a)
    return a.ctypes.data_as(i32p)


class Rig:
    """Every object the table's calls name, on one stream, and the good call that follows each refusal."""

    def __init__(self, capi):
        import torch

        self.capi, self.L, self.torch = capi, capi.load(), torch
        self.keep = []
        self.side = torch.cuda.Stream()
        s = self.stream = self.side.cuda_stream
        cu8, f32 = capi.DDC_CU8, capi.DDC_F32
        self.taps, self.ftaps = _taps(T, 15), _taps(FT, 16)

        def on(o):
            o.set_stream(s)
            return o

        self.ddc = on(capi.Ddc(D, self.taps, STEPS, in_format=cu8, max_in_samples=CAP))
        self.chan = on(capi.Chan(4, D, self.taps, (3, 0), in_format=cu8, max_in_samples=CAP))
        self.fine = on(capi.Fine(2, FD, self.ftaps, STEPS, inputs=(1, 0), max_in_samples=FCAP))
        self.nb = on(capi.Nb(cu8, B, W, 64, 3, max_in_samples=NB_CAP))
        # formats that have no correction or no sums
        self.ddc_f32 = on(capi.Ddc(D, self.taps, STEPS, in_format=f32, max_in_samples=CAP))
        self.ddc_real = on(capi.Ddc(D, self.taps, STEPS, in_format=capi.DDC_RU8, max_in_samples=CAP))
        self.chan_f32 = on(capi.Chan(4, D, self.taps, (3, 0), in_format=f32, max_in_samples=CAP))
        self.chan_real = on(capi.Chan(4, D, self.taps, (3, 0), in_format=capi.DDC_RS16, max_in_samples=CAP))
        # the chain's own members (a member driven directly is refused by its chain) and the ones that do not fit
        bank = dict(n_bands=2, max_batch_frames=64, max_listeners=2)
        self.c_nb = on(capi.Nb(cu8, B, W, 64, 3, max_in_samples=CAP))
        self.c_ddc = on(capi.Ddc(D, self.taps, STEPS, in_format=cu8, max_in_samples=CAP))
        self.c_fine = on(capi.Fine(2, FD, self.ftaps, STEPS, max_in_samples=FCAP))
        self.c_bank = on(capi.Bank(BANK_RATE, BANK_N, hop=BANK_HOP, **bank))
        self.chain = capi.Chain(self.c_bank, ddc=self.c_ddc, nb=self.c_nb, fine=self.c_fine, max_in_samples=CHAIN_MAX)
        self.nb_cs8 = on(capi.Nb(capi.DDC_CS8, B, W, 64, 3, max_in_samples=CAP))
        self.fine3 = on(capi.Fine(3, FD, self.ftaps, STEPS, inputs=(1, 0), max_in_samples=FCAP))
        self.c_chan = on(capi.Chan(4, D, self.taps, (3, 0), in_format=cu8, max_in_samples=CAP))
        self.bank1 = on(capi.Bank(BANK_RATE, BANK_N, n_bands=1, max_batch_frames=64, max_listeners=2, hop=BANK_HOP))
        self.ddc_null = capi.Ddc(D, self.taps, STEPS, in_format=cu8, max_in_samples=CAP)  # stays on the null stream
        self.ddc_tiny = on(capi.Ddc(D, self.taps, STEPS, in_format=cu8, max_in_samples=8))
        self.bank_graph = on(capi.Bank(BANK_RATE, BANK_N, **bank))
        self.bank_graph.graph_capture(4)
        self.bank_staged = on(capi.Bank(BANK_RATE, BANK_N, hop=BANK_HOP, **bank))
        assert self.bank_staged.push_iq(0, BANK_RATE, np.zeros((BANK_HOP, 2), np.float32)) == capi.OK
        self.bank_defer = on(capi.Bank(BANK_RATE, BANK_N, hop=BANK_HOP, **bank))
        self.bank_defer.enable_results(True)
        self.bank_defer.defer_listen(True)
        # a second chain, for the member that is driven directly
        self.d_ddc = on(capi.Ddc(D, self.taps, STEPS, in_format=cu8, max_in_samples=CAP))
        self.d_bank = on(capi.Bank(BANK_RATE, BANK_N, hop=BANK_HOP, **bank))
        self.driven = capi.Chain(self.d_bank, ddc=self.d_ddc, max_in_samples=CHAIN_MAX)

        with torch.cuda.stream(self.side):
            self.raw = torch.zeros((2 * NB_CAP + 16, 2), dtype=torch.uint8, device="cuda")     # raw cu8 input
            self.clean = torch.zeros((NB_CAP + 8, 2), dtype=torch.uint8, device="cuda")        # the blanker's output
            self.mid = torch.zeros((2, FCAP + 8, 2), dtype=torch.float32, device="cuda")       # the fine converter's inputs
            self.out = torch.zeros((2, OUT_STRIDE + 4, 2), dtype=torch.float32, device="cuda")
        self.side.synchronize()
        self.host = np.zeros((NB_CAP, 2), np.uint8)
        self.count = dict(ddc=0, chan=0, fine=0, nb=0, chain=0)

    def total(self, key):
        return self.chain.stats()["accepted"] if key == "chain" else getattr(self, key).total_samples

    def good(self, key):
        """One good call of the object; its sample count moves by exactly that call."""
        r, i, o = self, self.raw.data_ptr(), self.out.data_ptr()
        if key == "ddc":
            r.ddc.process_device(i, PIECE, o, OUT_STRIDE)
            n = PIECE
        elif key == "chan":
            r.chan.process_device(i, PIECE, o, OUT_STRIDE)
            n = PIECE
        elif key == "fine":
            r.fine.process_device(r.mid.data_ptr(), FCAP + 8, PIECE, o, OUT_STRIDE)
            n = PIECE
        elif key == "nb":
            r.nb.process_device(i, B, r.clean.data_ptr())
            n = B
        else:
            r.chain.push_host(r.host[:G])
            n = G
        getattr(r, key).sync()
        r.count[key] += n
        assert r.total(key) == r.count[key], key

    def close(self):
        self.chain.close()
        self.driven.close()
        self.bank_graph.graph_release()
        for name in ("ddc", "chan", "fine", "nb", "ddc_f32", "ddc_real", "chan_f32", "chan_real", "c_nb", "c_ddc", "c_fine", "c_bank",
                     "nb_cs8", "fine3", "c_chan", "bank1", "ddc_null", "ddc_tiny", "bank_graph", "bank_staged", "bank_defer", "d_ddc",
                     "d_bank"):
            getattr(self, name).close()


def cases(r):
    """[(id, the object whose good call follows, call, arguments...)]: in the order they run."""
    capi, L, keep = r.capi, r.L, r.keep
    tp, ftp = r.taps.ctypes.data_as(fp), r.ftaps.ctypes.data_as(fp)
    sp = _ints(keep, *STEPS)
    h = r.h = vp()
    hp = C.byref(h)
    raw, out, clean, mid = r.raw.data_ptr(), r.out.data_ptr(), r.clean.data_ptr(), r.mid.data_ptr()
    i_ok, o_ok, c_ok, m_ok = vp(raw), vp(out), vp(clean), vp(mid)
    host = vp(r.host.ctypes.data)
    t = []

    # -- the down-converter ---------------------------------------------------------------------------------------------------
    def dcfg(**kw):
        c = capi.DdcConfig(C.sizeof(capi.DdcConfig), len(STEPS), D, T, capi.DDC_CU8, CAP, 0, 0)
        for k, v in kw.items():
            setattr(c, k, v)
        keep.append(c)
        return C.byref(c)

    create = L.sdr_ddc_create
    for name, kw in (("struct_size", dict(struct_size=28)), ("decimation_0", dict(decimation=0)),
                     ("decimation_257", dict(decimation=257, max_in_samples=257)), ("n_taps_0", dict(n_taps=0)),
                     ("n_taps_4097", dict(n_taps=4097)), ("n_bands_0", dict(n_bands=0)), ("n_bands_65", dict(n_bands=65)),
                     ("format_4", dict(in_format=4)), ("format_neg", dict(in_format=-1)), ("max_in_ragged", dict(max_in_samples=CAP + 1)),
                     ("max_in_0", dict(max_in_samples=0)), ("reserved", dict(reserved=1))):
        t.append((f"ddc.create.{name}", "ddc", create, dcfg(**kw), tp, sp, hp))
    t += [
        ("ddc.create.null_config", "ddc", create, None, tp, sp, hp),
        ("ddc.create.null_taps", "ddc", create, dcfg(), None, sp, hp),
        ("ddc.create.null_steps", "ddc", create, dcfg(), tp, None, hp),
        ("ddc.create.null_out", "ddc", create, dcfg(), tp, sp, None),
        ("ddc.create.step_32768", "ddc", create, dcfg(), tp, _ints(keep, 100, 32768), hp),
        ("ddc.create.step_-32769", "ddc", create, dcfg(), tp, _ints(keep, -32769, 0), hp),
        ("ddc.create.null_config+bad_struct", "ddc", create, None, None, None, None),
    ]
    for obj, key, dev, hostcall, handle in (("ddc", "ddc", L.sdr_ddc_process_device, L.sdr_ddc_process_host, r.ddc._h),
                                            ("chan", "chan", L.sdr_chan_process_device, L.sdr_chan_process_host, r.chan._h)):
        t += [
            (f"{obj}.device.misaligned_in", key, dev, handle, vp(raw + 2), PIECE, o_ok, OUT_STRIDE),
            (f"{obj}.device.misaligned_out", key, dev, handle, i_ok, PIECE, vp(out + 8), OUT_STRIDE),
            (f"{obj}.device.null_in", key, dev, handle, None, PIECE, o_ok, OUT_STRIDE),
            (f"{obj}.device.null_out", key, dev, handle, i_ok, PIECE, None, OUT_STRIDE),
            (f"{obj}.device.null_handle", key, dev, None, i_ok, PIECE, o_ok, OUT_STRIDE),
            (f"{obj}.device.ragged", key, dev, handle, i_ok, PIECE + 1, o_ok, OUT_STRIDE),
            (f"{obj}.device.zero", key, dev, handle, i_ok, 0, o_ok, OUT_STRIDE),
            (f"{obj}.device.above_max_in", key, dev, handle, i_ok, CAP + D, o_ok, 20),
            (f"{obj}.device.stride_below", key, dev, handle, i_ok, 2 * PIECE, o_ok, 4),
            (f"{obj}.device.stride_not_4", key, dev, handle, i_ok, PIECE, o_ok, 10),
            (f"{obj}.host.ragged", key, hostcall, handle, host, D + 1, o_ok, OUT_STRIDE),
            (f"{obj}.host.null_in", key, hostcall, handle, None, PIECE, o_ok, OUT_STRIDE),
            (f"{obj}.host.misaligned_out", key, hostcall, handle, host, PIECE, vp(out + 8), OUT_STRIDE),
            (f"{obj}.host.stride_below", key, hostcall, handle, host, 2 * PIECE, o_ok, 4),
            # wrong in two ways
            (f"{obj}.device.null_handle+ragged", key, dev, None, i_ok, PIECE + 1, o_ok, OUT_STRIDE),
            (f"{obj}.device.null_in+zero", key, dev, handle, None, 0, o_ok, OUT_STRIDE),
            (f"{obj}.device.ragged+misaligned_in", key, dev, handle, vp(raw + 2), PIECE + 1, o_ok, OUT_STRIDE),
            (f"{obj}.device.above_max_in+misaligned_out", key, dev, handle, i_ok, CAP + D, vp(out + 8), 20),
            (f"{obj}.device.misaligned_in+stride_not_4", key, dev, handle, vp(raw + 2), PIECE, o_ok, 10),
            (f"{obj}.device.misaligned_out+stride_below", key, dev, handle, i_ok, 2 * PIECE, vp(out + 8), 4),
            (f"{obj}.host.ragged+misaligned_out", key, hostcall, handle, host, D + 1, vp(out + 8), OUT_STRIDE),
            (f"{obj}.host.misaligned_out+stride_not_4", key, hostcall, handle, host, PIECE, vp(out + 8), 10),
        ]
        prefix = f"sdr_{obj}"
        t += [
            (f"{obj}.sync.null", key, getattr(L, prefix + "_sync"), None),
            (f"{obj}.set_stream.null", key, getattr(L, prefix + "_set_stream"), None, None),
            (f"{obj}.set_first_sample.null", key, getattr(L, prefix + "_set_first_sample"), None, 0),
            (f"{obj}.set_first_sample.null+negative", key, getattr(L, prefix + "_set_first_sample"), None, -1),
            (f"{obj}.set_first_sample.started", key, getattr(L, prefix + "_set_first_sample"), handle, 4 * D),
            (f"{obj}.set_first_sample.started+negative", key, getattr(L, prefix + "_set_first_sample"), handle, -D),
        ]
    t += [
        ("ddc.set_nco_step.band_2", "ddc", L.sdr_ddc_set_nco_step, r.ddc._h, 2, 5),
        ("ddc.set_nco_step.band_neg", "ddc", L.sdr_ddc_set_nco_step, r.ddc._h, -1, 5),
        ("ddc.set_nco_step.step_32768", "ddc", L.sdr_ddc_set_nco_step, r.ddc._h, 0, 32768),
        ("ddc.set_nco_step.step_-32769", "ddc", L.sdr_ddc_set_nco_step, r.ddc._h, 0, -32769),
        ("ddc.set_nco_step.null", "ddc", L.sdr_ddc_set_nco_step, None, 0, 5),
        ("ddc.set_nco_step.band_2+step_32768", "ddc", L.sdr_ddc_set_nco_step, r.ddc._h, 2, 32768),
    ]

    # -- the channelizer ------------------------------------------------------------------------------------------------------
    def ccfg(**kw):
        c = capi.ChanConfig(C.sizeof(capi.ChanConfig), 4, D, T, capi.DDC_CU8, CAP, 0, 2)
        for k, v in kw.items():
            setattr(c, k, v)
        keep.append(c)
        return C.byref(c)

    create = L.sdr_chan_create
    cp = _ints(keep, 3, 0)
    for name, kw in (("struct_size", dict(struct_size=28)), ("n_channels_0", dict(n_channels=0)),
                     ("n_channels_1", dict(n_channels=1, decimation=1, n_taps=16, n_out=1)),
                     ("n_channels_6", dict(n_channels=6, decimation=6, n_taps=12)),
                     ("n_channels_512", dict(n_channels=512, decimation=512, n_taps=512, max_in_samples=512)),
                     ("decimation_0", dict(decimation=0)), ("decimation_m_8", dict(n_channels=8, decimation=1)),
                     ("decimation_2m", dict(decimation=8)), ("decimation_3", dict(decimation=3, max_in_samples=3 * 16)),
                     ("n_taps_0", dict(n_taps=0)), ("n_taps_ragged", dict(n_taps=T + 1)), ("n_taps_65m", dict(n_taps=65 * 4)),
                     ("n_taps_above_4096", dict(n_channels=256, decimation=64, n_taps=4096 + 256)),
                     ("format_4", dict(in_format=4)), ("format_neg", dict(in_format=-1)), ("max_in_ragged", dict(max_in_samples=CAP + 1)),
                     ("max_in_0", dict(max_in_samples=0)), ("n_out_0", dict(n_out=0)), ("n_out_above", dict(n_out=5))):
        t.append((f"chan.create.{name}", "chan", create, ccfg(**kw), tp, cp, hp))
    t += [
        ("chan.create.null_config", "chan", create, None, tp, cp, hp),
        ("chan.create.null_taps", "chan", create, ccfg(), None, cp, hp),
        ("chan.create.null_out", "chan", create, ccfg(), tp, cp, None),
        ("chan.create.channels_twice", "chan", create, ccfg(), tp, _ints(keep, 3, 3), hp),
        ("chan.create.channel_above", "chan", create, ccfg(), tp, _ints(keep, 3, 4), hp),
        ("chan.create.channel_neg", "chan", create, ccfg(), tp, _ints(keep, -1, 0), hp),
        ("chan.create.format_4+max_in_0", "chan", create, ccfg(in_format=4, max_in_samples=0), tp, cp, hp),
    ]

    # -- the IQ correction and the sums on both -------------------------------------------------------------------------------
    def corr(*v):
        c = capi.IqCorrection(*v)
        keep.append(c)
        return C.byref(c)

    nan, inf = float("nan"), float("inf")
    sums = r.sums = capi.IqSums()
    for obj, plain, f32, real in (("ddc", r.ddc, r.ddc_f32, r.ddc_real), ("chan", r.chan, r.chan_f32, r.chan_real)):
        set_c, enable, read = (getattr(L, f"sdr_iq_{obj}_{m}") for m in ("set_correction", "enable_sums", "read_sums"))
        t += [
            (f"iq.{obj}.set_correction.null", obj, set_c, None, corr(0, 0, 1, 0)),
            (f"iq.{obj}.set_correction.nan_dc_re", obj, set_c, plain._h, corr(nan, 0, 1, 0)),
            (f"iq.{obj}.set_correction.inf_dc_im", obj, set_c, plain._h, corr(0, inf, 1, 0)),
            (f"iq.{obj}.set_correction.inf_gain", obj, set_c, plain._h, corr(0, 0, -inf, 0)),
            (f"iq.{obj}.set_correction.nan_cross", obj, set_c, plain._h, corr(0, 0, 1, nan)),
            (f"iq.{obj}.set_correction.real", obj, set_c, real._h, corr(0, 0, 1, 0)),
            (f"iq.{obj}.set_correction.real_none", obj, set_c, real._h, None),
            (f"iq.{obj}.set_correction.real+nan", obj, set_c, real._h, corr(nan, 0, 1, 0)),
            (f"iq.{obj}.enable_sums.null", obj, enable, None, 1),
            (f"iq.{obj}.enable_sums.f32", obj, enable, f32._h, 1),
            (f"iq.{obj}.enable_sums.real", obj, enable, real._h, 1),
            (f"iq.{obj}.enable_sums.f32_off", obj, enable, f32._h, 0),
            (f"iq.{obj}.read_sums.null", obj, read, None, C.byref(sums)),
            (f"iq.{obj}.read_sums.null_out", obj, read, plain._h, None),
            (f"iq.{obj}.read_sums.off", obj, read, plain._h, C.byref(sums)),
            (f"iq.{obj}.read_sums.null_out+off", obj, read, f32._h, None),
        ]
    t += [
        ("iq.from_sums.null_sums", "ddc", L.sdr_iq_correction_from_sums, None, capi.DDC_CU8, corr(0, 0, 1, 0)),
        ("iq.from_sums.null_out", "ddc", L.sdr_iq_correction_from_sums, C.byref(sums), capi.DDC_CU8, None),
        ("iq.from_sums.no_samples", "ddc", L.sdr_iq_correction_from_sums, C.byref(sums), capi.DDC_CU8, corr(0, 0, 1, 0)),
    ]

    # -- the fine converter ---------------------------------------------------------------------------------------------------
    def fcfg(**kw):
        c = capi.FineConfig(C.sizeof(capi.FineConfig), len(STEPS), 2, FD, FT, FCAP, 0, 0)
        for k, v in kw.items():
            setattr(c, k, v)
        keep.append(c)
        return C.byref(c)

    create = L.sdr_fine_create
    ip = _ints(keep, 1, 0)
    for name, kw in (("struct_size", dict(struct_size=28)), ("n_bands_0", dict(n_bands=0)), ("n_bands_65", dict(n_bands=65)),
                     ("n_inputs_0", dict(n_inputs=0)), ("n_inputs_257", dict(n_inputs=257)), ("decimation_0", dict(decimation=0)),
                     ("decimation_257", dict(decimation=257, max_in_samples=257)), ("n_taps_0", dict(n_taps=0)),
                     ("n_taps_4097", dict(n_taps=4097)), ("max_in_ragged", dict(max_in_samples=FCAP + 1)),
                     ("max_in_0", dict(max_in_samples=0)), ("reserved", dict(reserved=1))):
        t.append((f"fine.create.{name}", "fine", create, fcfg(**kw), ftp, sp, ip, hp))
    stride, f = FCAP + 8, r.fine._h
    dev = L.sdr_fine_process_device
    t += [
        ("fine.create.null_config", "fine", create, None, ftp, sp, ip, hp),
        ("fine.create.null_taps", "fine", create, fcfg(), None, sp, ip, hp),
        ("fine.create.null_steps", "fine", create, fcfg(), ftp, None, ip, hp),
        ("fine.create.null_out", "fine", create, fcfg(), ftp, sp, ip, None),
        ("fine.create.step_32768", "fine", create, fcfg(), ftp, _ints(keep, 100, 32768), ip, hp),
        ("fine.create.step_-32769", "fine", create, fcfg(), ftp, _ints(keep, -32769, 0), ip, hp),
        ("fine.create.input_above", "fine", create, fcfg(), ftp, sp, _ints(keep, 0, 2), hp),
        ("fine.create.input_neg", "fine", create, fcfg(), ftp, sp, _ints(keep, -1, 0), hp),
        ("fine.create.no_map_more_bands", "fine", create, fcfg(n_inputs=1), ftp, sp, None, hp),
        ("fine.create.step_32768+input_above", "fine", create, fcfg(), ftp, _ints(keep, 32768, 0), _ints(keep, 2, 0), hp),
        ("fine.device.misaligned_in", "fine", dev, f, vp(mid + 8), stride, PIECE, o_ok, OUT_STRIDE),
        ("fine.device.misaligned_out", "fine", dev, f, m_ok, stride, PIECE, vp(out + 8), OUT_STRIDE),
        ("fine.device.null_in", "fine", dev, f, None, stride, PIECE, o_ok, OUT_STRIDE),
        ("fine.device.null_out", "fine", dev, f, m_ok, stride, PIECE, None, OUT_STRIDE),
        ("fine.device.null_handle", "fine", dev, None, m_ok, stride, PIECE, o_ok, OUT_STRIDE),
        ("fine.device.ragged", "fine", dev, f, m_ok, stride, PIECE + 1, o_ok, OUT_STRIDE),
        ("fine.device.zero", "fine", dev, f, m_ok, stride, 0, o_ok, OUT_STRIDE),
        ("fine.device.above_max_in", "fine", dev, f, m_ok, stride, FCAP + FD, o_ok, 36),
        ("fine.device.in_stride_below", "fine", dev, f, m_ok, PIECE - 4, PIECE, o_ok, OUT_STRIDE),
        ("fine.device.in_stride_not_4", "fine", dev, f, m_ok, PIECE + 2, PIECE, o_ok, OUT_STRIDE),
        ("fine.device.out_stride_below", "fine", dev, f, m_ok, stride, PIECE, o_ok, 4),
        ("fine.device.out_stride_not_4", "fine", dev, f, m_ok, stride, PIECE, o_ok, 10),
        ("fine.device.null_handle+ragged", "fine", dev, None, m_ok, stride, PIECE + 1, o_ok, OUT_STRIDE),
        ("fine.device.ragged+misaligned_in", "fine", dev, f, vp(mid + 8), stride, PIECE + 1, o_ok, OUT_STRIDE),
        ("fine.device.misaligned_in+in_stride_not_4", "fine", dev, f, vp(mid + 8), PIECE + 2, PIECE, o_ok, OUT_STRIDE),
        ("fine.device.misaligned_out+out_stride_below", "fine", dev, f, m_ok, stride, PIECE, vp(out + 8), 4),
        ("fine.device.in_stride_below+out_stride_not_4", "fine", dev, f, m_ok, PIECE - 4, PIECE, o_ok, 10),
        ("fine.set_nco_step.band_2", "fine", L.sdr_fine_set_nco_step, f, 2, 5),
        ("fine.set_nco_step.band_neg", "fine", L.sdr_fine_set_nco_step, f, -1, 5),
        ("fine.set_nco_step.step_32768", "fine", L.sdr_fine_set_nco_step, f, 0, 32768),
        ("fine.set_nco_step.step_-32769", "fine", L.sdr_fine_set_nco_step, f, 0, -32769),
        ("fine.set_nco_step.null", "fine", L.sdr_fine_set_nco_step, None, 0, 5),
        ("fine.set_input.band_2", "fine", L.sdr_fine_set_input, f, 2, 1),
        ("fine.set_input.band_neg", "fine", L.sdr_fine_set_input, f, -1, 1),
        ("fine.set_input.input_2", "fine", L.sdr_fine_set_input, f, 0, 2),
        ("fine.set_input.input_neg", "fine", L.sdr_fine_set_input, f, 0, -1),
        ("fine.set_input.null", "fine", L.sdr_fine_set_input, None, 0, 1),
        ("fine.sync.null", "fine", L.sdr_fine_sync, None),
        ("fine.set_stream.null", "fine", L.sdr_fine_set_stream, None, None),
        ("fine.set_first_sample.null", "fine", L.sdr_fine_set_first_sample, None, 0),
        ("fine.set_first_sample.started", "fine", L.sdr_fine_set_first_sample, f, 4 * FD),
        ("fine.set_first_sample.started+ragged", "fine", L.sdr_fine_set_first_sample, f, FD + 1),
        ("fine.tune.null_channel", "fine", L.sdr_fine_tune, 8, 4, 0, None, _ints(keep, 0)),
        ("fine.tune.n_channels_6", "fine", L.sdr_fine_tune, 6, 6, 0, _ints(keep, 0), _ints(keep, 0)),
    ]

    # -- the blanker ----------------------------------------------------------------------------------------------------------
    def ncfg(**kw):
        v = dict(struct_size=C.sizeof(capi.NbConfig), in_format=capi.DDC_CU8, block=B, window=W, ratio_q4=64, hold=3, max_in_samples=NB_CAP,
                 device_id=0)
        v.update(kw)
        c = capi.NbConfig(*[v[k] for k, _ in capi.NbConfig._fields_])
        keep.append(c)
        return C.byref(c)

    create = L.sdr_nb_create
    for name, kw in (("struct_size", dict(struct_size=28)), ("format_f32", dict(in_format=capi.DDC_F32)),
                     ("format_rf32", dict(in_format=capi.DDC_RF32)), ("format_4", dict(in_format=4)), ("block_32", dict(block=32)),
                     ("block_96", dict(block=96)), ("block_8192", dict(block=8192)), ("window_0", dict(window=0)),
                     ("window_3", dict(window=3)), ("window_128", dict(window=128)), ("block_times_window", dict(block=4096, window=32)),
                     ("ratio_15", dict(ratio_q4=15)), ("ratio_16385", dict(ratio_q4=16385)), ("ratio_neg", dict(ratio_q4=-1)),
                     ("hold_neg", dict(hold=-1)), ("hold_above", dict(hold=B + 1)), ("max_in_0", dict(max_in_samples=0)),
                     ("max_in_ragged", dict(max_in_samples=B + 1)), ("format_f32+block_32", dict(in_format=capi.DDC_F32, block=32))):
        t.append((f"nb.create.{name}", "nb", create, ncfg(**kw), hp))
    nb, dev, hostcall = r.nb._h, L.sdr_nb_process_device, L.sdr_nb_process_host
    stats = r.stats = capi.NbStats()
    t += [
        ("nb.create.null_config", "nb", create, None, hp),
        ("nb.create.null_out", "nb", create, ncfg(), None),
        ("nb.device.null_handle", "nb", dev, None, i_ok, B, c_ok),
        ("nb.device.null_in", "nb", dev, nb, None, B, c_ok),
        ("nb.device.null_out", "nb", dev, nb, i_ok, B, None),
        ("nb.device.zero", "nb", dev, nb, i_ok, 0, c_ok),
        ("nb.device.ragged", "nb", dev, nb, i_ok, B + 1, c_ok),
        ("nb.device.half_block", "nb", dev, nb, i_ok, B // 2, c_ok),
        ("nb.device.above_max_in", "nb", dev, nb, i_ok, NB_CAP + B, c_ok),
        ("nb.device.misaligned_in", "nb", dev, nb, vp(raw + 2), B, c_ok),
        ("nb.device.misaligned_out", "nb", dev, nb, i_ok, B, vp(clean + 8)),
        ("nb.device.in_place", "nb", dev, nb, i_ok, 2 * B, i_ok),
        ("nb.device.overlap_behind", "nb", dev, nb, i_ok, 2 * B, vp(raw + 2 * B)),
        ("nb.device.overlap_in_front", "nb", dev, nb, vp(raw + 2 * B), 2 * B, i_ok),
        ("nb.device.null_handle+ragged", "nb", dev, None, i_ok, B + 1, c_ok),
        ("nb.device.ragged+misaligned_in", "nb", dev, nb, vp(raw + 2), B + 1, c_ok),
        ("nb.device.in_place+ragged", "nb", dev, nb, i_ok, B + 1, i_ok),
        ("nb.device.overlap+above_max_in", "nb", dev, nb, i_ok, NB_CAP + B, vp(raw + 2 * B)),
        ("nb.device.misaligned_out+overlap", "nb", dev, nb, i_ok, 2 * B, vp(raw + 8)),
        ("nb.host.null_in", "nb", hostcall, nb, None, B, c_ok),
        ("nb.host.ragged", "nb", hostcall, nb, host, B - 1, c_ok),
        ("nb.host.misaligned_out", "nb", hostcall, nb, host, B, vp(clean + 4)),
        ("nb.host.ragged+misaligned_out", "nb", hostcall, nb, host, B - 1, vp(clean + 4)),
        ("nb.set_threshold.null", "nb", L.sdr_nb_set_threshold, None, 64, 3),
        ("nb.set_threshold.ratio_8", "nb", L.sdr_nb_set_threshold, nb, 8, 3),
        ("nb.set_threshold.ratio_20000", "nb", L.sdr_nb_set_threshold, nb, 20000, 3),
        ("nb.set_threshold.hold_above", "nb", L.sdr_nb_set_threshold, nb, 64, B + 1),
        ("nb.set_threshold.hold_neg", "nb", L.sdr_nb_set_threshold, nb, 64, -1),
        ("nb.set_first_sample.started", "nb", L.sdr_nb_set_first_sample, nb, 2 * B),
        ("nb.set_first_sample.started+ragged", "nb", L.sdr_nb_set_first_sample, nb, B + 1),
        ("nb.set_first_sample.null", "nb", L.sdr_nb_set_first_sample, None, 0),
        ("nb.set_stream.null", "nb", L.sdr_nb_set_stream, None, None),
        ("nb.sync.null", "nb", L.sdr_nb_sync, None),
        ("nb.read_stats.null", "nb", L.sdr_nb_read_stats, None, C.byref(stats)),
        ("nb.read_stats.null_out", "nb", L.sdr_nb_read_stats, nb, None),
        ("nb.blank_host.null_in", "nb", L.sdr_nb_blank_host, ncfg(), None, B, host, None),
        ("nb.blank_host.bad_config", "nb", L.sdr_nb_blank_host, ncfg(block=32), host, B, vp(r.host.ctypes.data + 2 * B), None),
        ("nb.blank_host.ragged", "nb", L.sdr_nb_blank_host, ncfg(), host, B + 1, vp(r.host.ctypes.data + 4 * B), None),
        ("nb.blank_host.in_place", "nb", L.sdr_nb_blank_host, ncfg(), host, B, host, None),
        ("nb.blank_host.overlap", "nb", L.sdr_nb_blank_host, ncfg(), host, B, vp(r.host.ctypes.data + B), None),
        ("nb.blank_host.in_place+ragged", "nb", L.sdr_nb_blank_host, ncfg(), host, B + 1, host, None),
    ]

    # -- the chain ------------------------------------------------------------------------------------------------------------
    def hcfg(**kw):
        c = capi.ChainConfig(C.sizeof(capi.ChainConfig), CHAIN_MAX, 0, 0, r.c_nb._h, r.c_ddc._h, None, r.c_fine._h, r.c_bank._h)
        for k, v in kw.items():
            setattr(c, k, v._h if hasattr(v, "_h") else v)
        keep.append(c)
        return C.byref(c)

    create = L.sdr_chain_create
    for name, kw in (("struct_size", dict(struct_size=48)), ("reserved", dict(reserved=1)), ("max_in_0", dict(max_in_samples=0)),
                     ("no_bank", dict(bank=None)), ("both_stage_ones", dict(chan=r.c_chan)), ("no_stage_one", dict(ddc=None)),
                     ("nb_format", dict(nb=r.nb_cs8)), ("fine_inputs", dict(fine=r.fine3)), ("bank_bands", dict(bank=r.bank1)),
                     ("streams", dict(ddc=r.ddc_null)), ("no_granule_fits", dict(ddc=r.ddc_tiny)),
                     ("ring_below", dict(ring_samples=MIN_RING - 4)), ("ring_not_4", dict(ring_samples=MIN_RING + 2)),
                     ("bank_graph", dict(bank=r.bank_graph)), ("bank_staged", dict(bank=r.bank_staged)),
                     ("bank_defer", dict(bank=r.bank_defer)), ("reserved+no_bank", dict(reserved=1, bank=None)),
                     ("nb_format+bank_bands", dict(nb=r.nb_cs8, bank=r.bank1)), ("ring_below+bank_graph", dict(ring_samples=4, bank=r.bank_graph))):
        t.append((f"chain.create.{name}", "chain", create, hcfg(**kw), hp))
    ch = r.chain._h
    n_b = r.n_b = C.c_int(-5)
    nbp = C.byref(n_b)
    narrow = np.zeros(8, np.float32)
    keep.append(narrow)
    np_ = narrow.ctypes.data_as(fp)
    push_d, push_h, read = L.sdr_chain_push_device, L.sdr_chain_push_host, L.sdr_chain_read_narrow
    t += [
        ("chain.create.null_config", "chain", create, None, hp),
        ("chain.create.null_out", "chain", create, hcfg(), None),
        ("chain.push_device.ragged", "chain", push_d, ch, i_ok, G + 8, nbp),
        ("chain.push_device.misaligned", "chain", push_d, ch, vp(raw + 8), G, nbp),
        ("chain.push_device.null_in", "chain", push_d, ch, None, G, nbp),
        ("chain.push_device.null_handle", "chain", push_d, None, i_ok, G, nbp),
        ("chain.push_device.zero", "chain", push_d, ch, i_ok, 0, nbp),
        ("chain.push_device.above_max_in", "chain", push_d, ch, i_ok, CHAIN_MAX + G, nbp),
        ("chain.push_device.null_handle+ragged", "chain", push_d, None, i_ok, G + 8, nbp),
        ("chain.push_device.ragged+misaligned", "chain", push_d, ch, vp(raw + 8), G + 8, nbp),
        ("chain.push_host.zero", "chain", push_h, ch, host, 0, nbp),
        ("chain.push_host.above_max_in", "chain", push_h, ch, host, CHAIN_MAX + 1, nbp),
        ("chain.push_host.null_in", "chain", push_h, ch, None, 100, nbp),
        ("chain.push_host.null_in+zero", "chain", push_h, ch, None, 0, nbp),
        ("chain.read_narrow.in_front", "chain", read, ch, 0, -1, 4, np_),
        ("chain.read_narrow.behind", "chain", read, ch, 0, 0, 1 << 20, np_),
        ("chain.read_narrow.nothing", "chain", read, ch, 0, 0, 0, np_),
        ("chain.read_narrow.band_2", "chain", read, ch, 2, 0, 4, np_),
        ("chain.read_narrow.null_out", "chain", read, ch, 0, 0, 4, None),
        ("chain.read_narrow.band_2+nothing", "chain", read, ch, 2, 0, 0, np_),
        ("chain.stats.null_out", "chain", L.sdr_chain_stats, ch, None),
        ("chain.stats.null_handle", "chain", L.sdr_chain_stats, None, C.byref(capi.ChainCounts())),
        ("chain.sync.null", "chain", L.sdr_chain_sync, None),
        ("chain.set_stream.null", "chain", L.sdr_chain_set_stream, None, None),
    ]
    return t


def pending_cases(r):
    """With samples of a host push pending (the caller pushes one and the rest of the granule around these)."""
    ch, nbp, raw = r.chain._h, C.byref(r.n_b), r.raw.data_ptr()
    push_d = r.L.sdr_chain_push_device
    return [
        ("chain.push_device.pending", "chain", push_d, ch, vp(raw), G, nbp),
        ("chain.push_device.pending+misaligned", "chain", push_d, ch, vp(raw + 8), G, nbp),
        ("chain.push_device.pending+ragged", "chain", push_d, ch, vp(raw), G + 8, nbp),
    ]


def driven_cases(r):
    """Behind a direct call of the second chain's down-converter: the chain refuses from then on."""
    ch, nbp = r.driven._h, C.byref(r.n_b)
    return [
        ("chain.push_host.member_driven", None, r.L.sdr_chain_push_host, ch, vp(r.host.ctypes.data), 100, nbp),
        ("chain.push_device.member_driven", None, r.L.sdr_chain_push_device, ch, vp(r.raw.data_ptr()), G, nbp),
        ("chain.push_device.member_driven+ragged", None, r.L.sdr_chain_push_device, ch, vp(r.raw.data_ptr()), G + 8, nbp),
    ]


def run(capi, on_case):
    """Runs the table: on_case(id, status, text) for every refusal; a good call in front of the first and behind each."""
    r = Rig(capi)
    L = r.L

    def refuse(case):
        name, key, call, *args = case
        r.h.value = 0xdead
        status = call(*args)
        text = L.sdr_last_error().decode()
        assert r.h.value == 0xdead and r.n_b.value == -5, name
        if key:
            assert r.total(key) == r.count[key], name  # (the refusal left the object where it was)
        on_case(name, status, text)
        if key:
            r.good(key)

    table = cases(r)
    for key in r.count:
        r.good(key)
    for case in table:
        refuse(case)
    # the chain with samples pending: one sample of a host push in front, the rest of its granule behind
    r.chain.push_host(r.host[:1])
    r.count["chain"] += 1
    for name, key, call, *args in pending_cases(r):
        status = call(*args)
        on_case(name, status, L.sdr_last_error().decode())
        assert r.n_b.value == -5 and r.total("chain") == r.count["chain"], name
    r.chain.push_host(r.host[:G - 1])
    r.count["chain"] += G - 1
    r.good("chain")
    assert r.chain.stats()["pending"] == 0
    # a member driven directly
    r.driven.push_host(r.host[:G])
    r.d_ddc.process_device(r.raw.data_ptr(), PIECE, r.out.data_ptr(), OUT_STRIDE)
    r.d_ddc.sync()
    for case in driven_cases(r):
        refuse(case)
    assert r.driven.stats()["accepted"] == G
    ids = [c[0] for c in table + pending_cases(r) + driven_cases(r)]
    assert len(set(ids)) == len(ids)
    r.close()
    return ids


def record():
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from sdrainer_amd import capi

    capi.load()
    got = {}

    def keep(name, status, text):
        assert status != capi.OK and text, f"{name} was not refused"
        got[name] = [status, text]

    run(capi, keep)
    with open(GOLDEN, "w") as f:
        json.dump(got, f, indent=1)
        f.write("\n")
    print(f"{len(got)} refusals -> {GOLDEN}")


if __name__ == "__main__":
    record()
