"""ctypes binding of libsdrainer_hip.so — the same C ABI (include/sdrainer_hip.h) a cgo shim binds.

There is no CPU implementation behind this module: if the HIP library is missing or fails to load,
importing raises.  PyTorch is only used by callers for device memory / streams; the ABI takes raw
device pointers.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SDR_HIP_LIB") or os.path.join(_HERE, "csrc", "libsdrainer_hip.so")  # env: diagnostic builds

OK, ERR_BAD_ARG, ERR_BAD_RATE, ERR_BAD_SIZE, ERR_WOULD_DROP, ERR_HIP, ERR_NO_SLOT, ERR_STATE, ERR_WOULD_BLOCK = range(9)
CUMULATION_SIZE = 100
KERNELS = ("k_fft_psd", "k_window_means", "k_noise_stats", "k_thresholds", "k_listen_gather", "k_cumulate",
           "k_find_peaks", "k_listen_decode")
REPORT_KERNELS = ("k_listen_report", "k_report_marks")  # profile slots 9 and 10 (launched only while reports are on: Bank.enable_reports)
ROWS_KERNEL = "k_cum_rows"  # profile slot 8, behind the eight stages (launched only while rows are on: Bank.enable_rows)


class SdrError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libsdrainer_hip status {code}: {msg}")
        self.code = code


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("n_bands", C.c_int32), ("sample_rate", C.c_int32), ("block_size", C.c_int32),
        ("edge_width", C.c_int32), ("peak_threshold", C.c_float), ("signal_debounce", C.c_int32),
        ("max_listeners", C.c_int32), ("max_batch_frames", C.c_int32), ("max_peaks", C.c_int32),
        ("find_peaks", C.c_int32), ("trace", C.c_int32), ("device_id", C.c_int32),
        # sdr_config.hop (0 = block_size).  The name keeps its `reserved` prefix: the field took the place of the struct's
        # reserved word, and the layout walk of tests/test_capi_c.py passes over names that start with it (the C program it
        # compares with predates the field; tests/host/test_overlap_layout.c prints this one).  Config.hop reads / writes it.
        ("reserved_hop", C.c_int32),
    ]

    @property
    def hop(self) -> int:
        return self.reserved_hop

    @hop.setter
    def hop(self, value: int):
        self.reserved_hop = value


class Peak(C.Structure):
    _fields_ = [
        ("from_", C.c_int32), ("to", C.c_int32), ("from_frequency", C.c_int64), ("to_frequency", C.c_int64),
        ("signal_frequency", C.c_int64), ("signal_value", C.c_float), ("signal_bin", C.c_int32),
    ]

    def astuple(self):
        return (self.from_, self.to, self.from_frequency, self.to_frequency, self.signal_frequency,
                float(np.float32(self.signal_value)), self.signal_bin)


FRAME_REC_DTYPE = np.dtype([("min_mean", "<f4"), ("dev_in", "<f4"), ("variance", "<f8"), ("nf_in", "<f4"),
                            ("noise_dev", "<f4"), ("noise_floor", "<f4"), ("peak_thr", "<f4"), ("listen_thr", "<f4"),
                            ("pad", "<f4")])
EDGE_DTYPE = np.dtype([("frame", "<u4"), ("state", "<u4")])
PEAK_DTYPE = np.dtype([("from", "<i4"), ("to", "<i4"), ("from_frequency", "<i8"), ("to_frequency", "<i8"),
                       ("signal_frequency", "<i8"), ("signal_value", "<f4"), ("signal_bin", "<i4")])
CHUNK_RESULT_DTYPE = np.dtype([("band", "<i4"), ("n_peaks", "<i4"), ("frame", "<i8"), ("first_peak", "<i4"),
                               ("peaks_found", "<i4")])
LISTENER_RESULT_DTYPE = np.dtype([("band", "<i4"), ("listener", "<i4"), ("first_edge", "<i4"), ("n_edges", "<i4"),
                                  ("first_rune", "<i4"), ("n_runes", "<i4")])


# sdr_listener_report (64 bytes): one listener's level, noise floor and speed over one batch, as sums that add up
REPORT_DTYPE = np.dtype([("band", "<i4"), ("listener", "<i4"), ("bin", "<i4"), ("ticks", "<i4"), ("ticks_on", "<i4"),
                         ("ticks_off", "<i4"), ("on_max_q", "<i4"), ("reserved", "<i4"), ("on_sum_q", "<i8"), ("off_sum_q", "<i8"),
                         ("floor_sum_q", "<i8"), ("wpm", "<f8")])
assert REPORT_DTYPE.itemsize == 64


def report_snr_db(reports) -> np.ndarray:
    """The mean key-down level over the band's noise floor in dB, per record: (on_sum_q - floor_sum_q) / (256 ticks_on);
    NaN where a listener had no measured key-down tick."""
    reports = np.asarray(reports)
    on = reports["ticks_on"].astype(np.float64)
    diff = (reports["on_sum_q"] - reports["floor_sum_q"]).astype(np.float64)
    return np.where(on > 0, diff / (256.0 * np.maximum(on, 1.0)), np.nan)


class ScopeSpectralFrame(C.Structure):
    """sdr_scope_spectral_frame: scope.SpectralFrame without its Values (scope/scope.go:24-31)."""
    _fields_ = [("frame", C.c_int64), ("from_frequency", C.c_double), ("to_frequency", C.c_double),
                ("signal_bin", C.c_double), ("threshold", C.c_double), ("n_values", C.c_int32), ("reserved", C.c_int32)]


SCOPE_TIME_DTYPE = np.dtype([("threshold", "<f8"), ("value", "<f8"), ("state", "<f8"), ("debounced", "<f8")])
SCOPE_DECODE_DTYPE = np.dtype([("frame", "<i8"), ("duration", "<f8"), ("state", "<f8"), ("on_threshold", "<f8"),
                               ("on_threshold_low", "<f8"), ("on_threshold_high", "<f8"), ("off_threshold", "<f8"),
                               ("off_threshold_low", "<f8"), ("off_threshold_high", "<f8")])


class Results(C.Structure):
    """sdr_results (include/sdrainer_hip.h)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("n_frames", C.c_int32), ("batch_index", C.c_int64), ("first_frame", C.c_int64),
        ("chunks", C.c_void_p), ("chunks_cap", C.c_int32), ("n_chunks", C.c_int32),
        ("peaks", C.c_void_p), ("peaks_cap", C.c_int32), ("n_peaks", C.c_int32),
        ("listeners", C.c_void_p), ("listeners_cap", C.c_int32), ("n_listeners", C.c_int32),
        ("edges", C.c_void_p), ("edges_cap", C.c_int32), ("n_edges", C.c_int32),
        ("runes", C.c_void_p), ("rune_frames", C.c_void_p), ("runes_cap", C.c_int32), ("n_runes", C.c_int32),
        ("runes_dropped", C.c_uint64), ("edges_dropped", C.c_uint64),
    ]

_lib = None


def _set_window(fn, handle, w):
    if w is None:
        return fn(handle, None, 0)
    w = np.ascontiguousarray(w, np.float32).reshape(-1)
    return fn(handle, w.ctypes.data_as(C.POINTER(C.c_float)), int(w.size))

# 8-bit input formats (SDR_IQ8_CS8 / SDR_IQ8_CU8)
IQ8_CS8, IQ8_CU8 = 0, 1


# the down-converter (sdr_ddc_*): input formats, the NCO table's size, the outputs of one band per workgroup
DDC_F32, DDC_SC16, DDC_CS8, DDC_CU8 = range(4)
# real input, one value per sample: the flag, and the flag with each sample type
DDC_REAL = 16
DDC_RF32, DDC_RS16, DDC_RS8, DDC_RU8 = (DDC_REAL | f for f in (DDC_F32, DDC_SC16, DDC_CS8, DDC_CU8))
DDC_NCO_SIZE = 65536
DDC_TILE_OUTPUTS = 512


class DdcConfig(C.Structure):
    """sdr_ddc_config (include/sdrainer_hip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("n_bands", C.c_int32), ("decimation", C.c_int32), ("n_taps", C.c_int32),
                ("in_format", C.c_int32), ("max_in_samples", C.c_int32), ("device_id", C.c_int32), ("reserved", C.c_int32)]


class ChanConfig(C.Structure):
    """sdr_chan_config (include/sdrainer_hip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("n_channels", C.c_int32), ("decimation", C.c_int32), ("n_taps", C.c_int32),
                ("in_format", C.c_int32), ("max_in_samples", C.c_int32), ("device_id", C.c_int32), ("n_out", C.c_int32)]


class IqCorrection(C.Structure):
    """sdr_iq_correction (include/sdrainer_hip.h): re = re0 - dc_re, im = gain_im * (im0 - dc_im) + cross * re."""
    _fields_ = [("dc_re", C.c_float), ("dc_im", C.c_float), ("gain_im", C.c_float), ("cross", C.c_float)]

    def astuple(self):
        return (self.dc_re, self.dc_im, self.gain_im, self.cross)


IQ_SUMS_FIELDS = ("n", "sum_i", "sum_q", "sum_ii", "sum_qq", "sum_iq", "skipped", "reserved")


class IqSums(C.Structure):
    """sdr_iq_sums (include/sdrainer_hip.h): exact sums of the raw stream in integer units (cs8 x, cu8 2 x - 255, sc16 x)."""
    _fields_ = [(f, C.c_int64) for f in IQ_SUMS_FIELDS]

    def asdict(self) -> dict:
        return {f: int(getattr(self, f)) for f in IQ_SUMS_FIELDS}


def _iq_correction(c):
    """None, an IqCorrection or four numbers (dc_re, dc_im, gain_im, cross) -> the pointer argument."""
    if c is None:
        return None
    return C.byref(c if isinstance(c, IqCorrection) else IqCorrection(*[float(v) for v in c]))


def _iq_sums(s) -> IqSums:
    return s if isinstance(s, IqSums) else IqSums(**{f: int(s.get(f, 0)) for f in IQ_SUMS_FIELDS})


def iq_correction_from_sums(sums, in_format: int) -> IqCorrection:
    """sdr_iq_correction_from_sums: the blind estimate of DC offset and imbalance from a stream's sums (an IqSums or a dict
    of its fields).  Needs no GPU.  SdrError(ERR_BAD_ARG) where the sums give none."""
    out = IqCorrection()
    _check(load().sdr_iq_correction_from_sums(C.byref(_iq_sums(sums)), int(in_format), C.byref(out)))
    return out


class NbConfig(C.Structure):
    """sdr_nb_config (include/sdrainer_hip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("in_format", C.c_int32), ("block", C.c_int32), ("window", C.c_int32),
                ("ratio_q4", C.c_int32), ("hold", C.c_int32), ("max_in_samples", C.c_int32), ("device_id", C.c_int32)]


class FineConfig(C.Structure):
    """sdr_fine_config (include/sdrainer_hip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("n_bands", C.c_int32), ("n_inputs", C.c_int32), ("decimation", C.c_int32),
                ("n_taps", C.c_int32), ("max_in_samples", C.c_int32), ("device_id", C.c_int32), ("reserved", C.c_int32)]


class ChainConfig(C.Structure):
    """sdr_chain_config (include/sdrainer_hip.h): the handles are borrowed."""
    _fields_ = [("struct_size", C.c_int32), ("max_in_samples", C.c_int32), ("ring_samples", C.c_int32), ("reserved", C.c_int32),
                ("nb", C.c_void_p), ("ddc", C.c_void_p), ("chan", C.c_void_p), ("fine", C.c_void_p), ("bank", C.c_void_p)]


CHAIN_COUNT_FIELDS = ("accepted", "processed", "pending", "narrow", "frames", "batches", "carry_moves", "granule", "piece",
                      "ring_samples", "resident_from", "reserved")


class ChainCounts(C.Structure):
    """sdr_chain_counts (include/sdrainer_hip.h): what sdr_chain_stats reports."""
    _fields_ = [(f, C.c_int64) for f in CHAIN_COUNT_FIELDS]

    def asdict(self) -> dict:
        return {f: int(getattr(self, f)) for f in CHAIN_COUNT_FIELDS}


NB_STATS_FIELDS = ("samples", "impulses", "blanked", "reserved")


class NbStats(C.Structure):
    """sdr_nb_stats (include/sdrainer_hip.h): samples seen, samples judged impulses, samples replaced."""
    _fields_ = [(f, C.c_int64) for f in NB_STATS_FIELDS]

    def asdict(self) -> dict:
        return {f: int(getattr(self, f)) for f in NB_STATS_FIELDS}


def _iq8_bytes(iq, fmt):
    """The bytes of an 8-bit push: int8 for cs8, uint8 for cu8 (any other fmt goes to the library, which refuses it)."""
    return np.ascontiguousarray(iq, dtype=np.int8 if fmt == IQ8_CS8 else np.uint8).reshape(-1)


# every symbol include/sdrainer_hip.h declares (tests/test_capi_symbols.py checks the header against this)
SYMBOLS = (
    "sdr_last_error sdr_abi_version sdr_create sdr_destroy sdr_self_check sdr_set_stream sdr_push_iq sdr_push_kiwi_snd sdr_staged_frames "
    "sdr_process_staged sdr_process_staged_limit sdr_process_device sdr_sync sdr_attach sdr_detach sdr_listener_count sdr_listener_stop "
    "sdr_set_peak_threshold sdr_set_edge_width sdr_set_signal_debounce sdr_set_center_frequency sdr_set_find_peaks "
    "sdr_last_batch_frames sdr_total_frames sdr_last_batch_chunks sdr_read_peaks sdr_read_cumulation sdr_read_text "
    "sdr_read_edges sdr_read_keying_bits sdr_read_frame_records sdr_read_trace sdr_read_spectrum "
    "sdr_read_decoder_state sdr_graph_batches sdr_graph_capture sdr_graph_launch sdr_graph_release sdr_scope_active sdr_scope_read_spectral sdr_scope_read_demod sdr_scope_read_decode sdr_enable_results sdr_poll sdr_defer_listen sdr_listen_pending sdr_poll_peaks sdr_attach_at sdr_process_listen sdr_results_pending sdr_read_drop_counters sdr_profile_enable sdr_profile_read sdr_profile_reset sdr_kernel_name sdr_audio_create "
    "sdr_group_create sdr_group_destroy sdr_group_member sdr_group_push_iq sdr_group_push_kiwi_snd sdr_group_process_staged "
    "sdr_group_process_staged_limit sdr_group_process_device sdr_group_sync sdr_group_set_peak_threshold "
    "sdr_group_set_signal_debounce sdr_group_set_edge_width sdr_group_set_find_peaks sdr_group_enable_results sdr_group_poll "
    "sdr_group_defer_listen sdr_group_poll_peaks sdr_group_process_listen sdr_group_read_drop_counters "
    "sdr_push_iq_sc16 sdr_process_device_sc16 sdr_graph_capture_sc16 sdr_graph_launch_sc16 "
    "sdr_group_push_iq_sc16 sdr_group_process_device_sc16 "
    "sdr_hop sdr_process_device_stream sdr_process_device_stream_sc16 "
    "sdr_push_iq8 sdr_process_device_iq8 sdr_process_device_stream_iq8 sdr_graph_capture_iq8 sdr_graph_launch_iq8 "
    "sdr_group_push_iq8 sdr_group_process_device_iq8 "
    "sdr_set_window sdr_group_set_window "
    "sdr_set_first_frame sdr_group_set_first_frame "
    "sdr_enable_rows sdr_row_columns sdr_poll_rows sdr_group_enable_rows sdr_group_poll_rows "
    "sdr_enable_reports sdr_reports_enabled sdr_poll_reports sdr_group_enable_reports sdr_group_poll_reports "
    "sdr_ddc_create sdr_ddc_destroy sdr_ddc_sync sdr_ddc_set_stream sdr_ddc_set_first_sample sdr_ddc_total_samples "
    "sdr_ddc_set_nco_step sdr_ddc_process_device sdr_ddc_process_host sdr_ddc_nco_table "
    "sdr_chan_create sdr_chan_destroy sdr_chan_sync sdr_chan_set_stream sdr_chan_set_first_sample sdr_chan_total_samples "
    "sdr_chan_process_device sdr_chan_process_host sdr_chan_tile_outputs "
    "sdr_iq_ddc_set_correction sdr_iq_ddc_enable_sums sdr_iq_ddc_read_sums "
    "sdr_iq_chan_set_correction sdr_iq_chan_enable_sums sdr_iq_chan_read_sums sdr_iq_correction_from_sums "
    "sdr_nb_create sdr_nb_destroy sdr_nb_sync sdr_nb_set_stream sdr_nb_set_first_sample sdr_nb_total_samples sdr_nb_set_threshold "
    "sdr_nb_process_device sdr_nb_process_host sdr_nb_read_stats sdr_nb_tile_samples sdr_nb_blank_host "
    "sdr_fine_create sdr_fine_destroy sdr_fine_sync sdr_fine_set_stream sdr_fine_set_first_sample sdr_fine_total_samples "
    "sdr_fine_set_nco_step sdr_fine_set_input sdr_fine_process_device sdr_fine_tune "
    "sdr_chain_create sdr_chain_destroy sdr_chain_set_stream sdr_chain_sync sdr_chain_push_host sdr_chain_push_device "
    "sdr_chain_read_narrow sdr_chain_stats sdr_chain_granule sdr_chain_min_ring "
    "sdr_audio_destroy sdr_audio_blocksize sdr_audio_set_scale sdr_audio_set_debounce "
    "sdr_audio_set_magnitude_threshold sdr_audio_write sdr_audio_close sdr_audio_read_text sdr_audio_read_trace"
).split()


def load():
    """Loads the HIP library.  Fails loudly: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m sdrainer_amd.csrc.build` (hipcc, gfx950). "
            "sdrainer_amd has no CPU fallback.")
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.7 / libhsa-runtime64.so.1.  Two HSA runtimes
    # in one process fight over the device ("No HIP GPUs are available" for whichever comes second),
    # so when torch is installed let it load its copy first: the dynamic loader then resolves this
    # library's libamdhip64.so.7 to the already-loaded one.  Without torch (e.g. under a cgo host) the
    # system ROCm runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, ip, fp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)

    def sig(name, res, *args):
        f = getattr(L, name)
        f.restype = res
        f.argtypes = list(args)

    sig("sdr_last_error", C.c_char_p)
    sig("sdr_abi_version", C.c_int)
    sig("sdr_create", C.c_int, C.POINTER(Config), C.POINTER(vp))
    sig("sdr_self_check", C.c_int, C.c_int)
    sig("sdr_destroy", C.c_int, vp)
    sig("sdr_set_stream", C.c_int, vp, vp)
    sig("sdr_push_iq", C.c_int, vp, C.c_int, C.c_int, fp, C.c_size_t)
    sig("sdr_push_kiwi_snd", C.c_int, vp, C.c_int, C.c_int, C.c_char_p, C.c_size_t)
    sig("sdr_staged_frames", C.c_int, vp, C.c_int)
    sig("sdr_process_staged", C.c_int, vp, ip)
    sig("sdr_process_staged_limit", C.c_int, vp, C.c_int, ip)
    sig("sdr_process_device", C.c_int, vp, vp, C.c_int)
    sig("sdr_push_iq_sc16", C.c_int, vp, C.c_int, C.c_int, C.POINTER(C.c_int16), C.c_size_t)
    sig("sdr_process_device_sc16", C.c_int, vp, vp, C.c_int)
    sig("sdr_hop", C.c_int, vp)
    sig("sdr_process_device_stream", C.c_int, vp, vp, C.c_int, C.c_size_t)
    sig("sdr_process_device_stream_sc16", C.c_int, vp, vp, C.c_int, C.c_size_t)
    sig("sdr_push_iq8", C.c_int, vp, C.c_int, C.c_int, vp, C.c_size_t, C.c_int)
    sig("sdr_process_device_iq8", C.c_int, vp, vp, C.c_int, C.c_int)
    sig("sdr_process_device_stream_iq8", C.c_int, vp, vp, C.c_int, C.c_size_t, C.c_int)
    sig("sdr_set_first_frame", C.c_int, vp, C.c_int64)
    sig("sdr_group_set_first_frame", C.c_int, vp, C.c_int64)
    sig("sdr_sync", C.c_int, vp)
    sig("sdr_attach", C.c_int, vp, C.c_int, C.c_int, ip)
    sig("sdr_detach", C.c_int, vp, C.c_int, C.c_int)
    sig("sdr_listener_count", C.c_int, vp, C.c_int)
    sig("sdr_listener_stop", C.c_int, vp, C.c_int, C.c_int)
    sig("sdr_set_peak_threshold", C.c_int, vp, C.c_int, C.c_float)
    sig("sdr_set_edge_width", C.c_int, vp, C.c_int)
    sig("sdr_set_signal_debounce", C.c_int, vp, C.c_int, C.c_int)
    sig("sdr_set_center_frequency", C.c_int, vp, C.c_int, C.c_int64)
    sig("sdr_set_find_peaks", C.c_int, vp, C.c_int)
    sig("sdr_set_window", C.c_int, vp, C.POINTER(C.c_float), C.c_int)
    sig("sdr_last_batch_frames", C.c_int, vp)
    sig("sdr_total_frames", C.c_int64, vp)
    sig("sdr_last_batch_chunks", C.c_int, vp)
    sig("sdr_read_peaks", C.c_int, vp, C.c_int, C.c_int, C.POINTER(Peak), C.c_int, ip, ip)
    sig("sdr_read_cumulation", C.c_int, vp, C.c_int, C.c_int, fp)
    sig("sdr_read_text", C.c_int, vp, C.c_int, C.c_int, C.c_char_p, C.c_int, ip)
    sig("sdr_read_edges", C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, ip)
    sig("sdr_read_keying_bits", C.c_int, vp, C.c_int, C.c_int, vp, C.c_int)
    sig("sdr_read_frame_records", C.c_int, vp, C.c_int, vp, C.c_int)
    sig("sdr_read_trace", C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int)
    sig("sdr_read_spectrum", C.c_int, vp, C.c_int, C.c_int, vp, vp)
    sig("sdr_read_decoder_state", C.c_int, vp, C.c_int, C.c_int, C.POINTER(C.c_double))
    sig("sdr_graph_batches", C.c_int, vp)
    sig("sdr_graph_capture", C.c_int, vp, C.c_int)
    sig("sdr_graph_launch", C.c_int, vp, C.POINTER(C.c_void_p))
    sig("sdr_graph_capture_sc16", C.c_int, vp, C.c_int)
    sig("sdr_graph_launch_sc16", C.c_int, vp, C.POINTER(C.c_void_p))
    sig("sdr_graph_capture_iq8", C.c_int, vp, C.c_int, C.c_int)
    sig("sdr_graph_launch_iq8", C.c_int, vp, C.POINTER(C.c_void_p), C.c_int)
    sig("sdr_graph_release", C.c_int, vp)
    sig("sdr_scope_active", C.c_int, vp)
    sig("sdr_scope_read_spectral", C.c_int, vp, C.c_int, C.c_int, C.POINTER(ScopeSpectralFrame), C.POINTER(C.c_double), C.c_int)
    sig("sdr_scope_read_demod", C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, ip)
    sig("sdr_scope_read_decode", C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, ip)
    sig("sdr_enable_results", C.c_int, vp, C.c_int)
    sig("sdr_poll", C.c_int, vp, C.POINTER(Results), C.c_int)
    sig("sdr_defer_listen", C.c_int, vp, C.c_int)
    sig("sdr_listen_pending", C.c_int, vp)
    sig("sdr_poll_peaks", C.c_int, vp, C.POINTER(Results), C.c_int)
    sig("sdr_attach_at", C.c_int, vp, C.c_int, C.c_int, C.c_int64, ip)
    sig("sdr_process_listen", C.c_int, vp)
    sig("sdr_results_pending", C.c_int, vp)
    sig("sdr_read_drop_counters", C.c_int, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
    sig("sdr_profile_enable", C.c_int, vp, C.c_int)
    sig("sdr_profile_read", C.c_int, vp, C.c_int, C.POINTER(C.c_double), ip)
    sig("sdr_profile_reset", C.c_int, vp)
    sig("sdr_kernel_name", C.c_char_p, C.c_int)
    sig("sdr_audio_create", C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.POINTER(vp))
    sig("sdr_audio_destroy", C.c_int, vp)
    sig("sdr_audio_blocksize", C.c_int, vp)
    sig("sdr_audio_set_scale", C.c_int, vp, C.c_double)
    sig("sdr_audio_set_debounce", C.c_int, vp, C.c_int)
    sig("sdr_audio_set_magnitude_threshold", C.c_int, vp, C.c_double)
    sig("sdr_audio_write", C.c_int, vp, fp, C.c_int)
    sig("sdr_audio_close", C.c_int, vp)
    sig("sdr_audio_read_text", C.c_int, vp, C.c_int, C.c_char_p, C.c_int, ip)
    sig("sdr_audio_read_trace", C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, ip)
    sig("sdr_group_create", C.c_int, C.POINTER(Config), C.POINTER(C.c_int32), C.c_int, C.POINTER(vp))
    sig("sdr_group_destroy", C.c_int, vp)
    sig("sdr_group_member", C.c_int, vp, C.c_int, C.POINTER(vp), ip)
    sig("sdr_group_push_iq", C.c_int, vp, C.c_int, C.c_int, fp, C.c_size_t)
    sig("sdr_group_push_kiwi_snd", C.c_int, vp, C.c_int, C.c_int, C.c_char_p, C.c_size_t)
    sig("sdr_group_process_staged", C.c_int, vp, ip)
    sig("sdr_group_process_staged_limit", C.c_int, vp, C.c_int, ip)
    sig("sdr_group_process_device", C.c_int, vp, C.POINTER(C.c_void_p), C.c_int)
    sig("sdr_group_push_iq_sc16", C.c_int, vp, C.c_int, C.c_int, C.POINTER(C.c_int16), C.c_size_t)
    sig("sdr_group_process_device_sc16", C.c_int, vp, C.POINTER(C.c_void_p), C.c_int)
    sig("sdr_group_push_iq8", C.c_int, vp, C.c_int, C.c_int, vp, C.c_size_t, C.c_int)
    sig("sdr_group_process_device_iq8", C.c_int, vp, C.POINTER(C.c_void_p), C.c_int, C.c_int)
    sig("sdr_group_sync", C.c_int, vp)
    sig("sdr_group_set_peak_threshold", C.c_int, vp, C.c_int, C.c_float)
    sig("sdr_group_set_signal_debounce", C.c_int, vp, C.c_int, C.c_int)
    sig("sdr_group_set_edge_width", C.c_int, vp, C.c_int)
    sig("sdr_group_set_find_peaks", C.c_int, vp, C.c_int)
    sig("sdr_group_set_window", C.c_int, vp, C.POINTER(C.c_float), C.c_int)
    sig("sdr_group_enable_results", C.c_int, vp, C.c_int)
    sig("sdr_group_poll", C.c_int, vp, C.POINTER(Results), C.c_int)
    sig("sdr_group_defer_listen", C.c_int, vp, C.c_int)
    sig("sdr_group_poll_peaks", C.c_int, vp, C.POINTER(Results), C.c_int)
    sig("sdr_group_process_listen", C.c_int, vp)
    sig("sdr_group_read_drop_counters", C.c_int, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))
    sig("sdr_enable_rows", C.c_int, vp, C.c_int)
    sig("sdr_row_columns", C.c_int, vp)
    sig("sdr_poll_rows", C.c_int, vp, fp, C.c_int, ip, C.POINTER(C.c_int64), C.c_int)
    sig("sdr_group_enable_rows", C.c_int, vp, C.c_int)
    sig("sdr_group_poll_rows", C.c_int, vp, fp, C.c_int, ip, C.POINTER(C.c_int64), C.c_int)
    sig("sdr_enable_reports", C.c_int, vp, C.c_int)
    sig("sdr_reports_enabled", C.c_int, vp)
    sig("sdr_poll_reports", C.c_int, vp, vp, C.c_int, ip, C.POINTER(C.c_int64), C.c_int)
    sig("sdr_group_enable_reports", C.c_int, vp, C.c_int)
    sig("sdr_group_poll_reports", C.c_int, vp, vp, C.c_int, ip, C.POINTER(C.c_int64), C.c_int)
    for obj in ("ddc", "chan", "nb", "fine"):  # what every front-end object has (_Front)
        sig(f"sdr_{obj}_destroy", C.c_int, vp)
        sig(f"sdr_{obj}_sync", C.c_int, vp)
        sig(f"sdr_{obj}_set_stream", C.c_int, vp, vp)
        sig(f"sdr_{obj}_set_first_sample", C.c_int, vp, C.c_int64)
        sig(f"sdr_{obj}_total_samples", C.c_int64, vp)
    sig("sdr_ddc_create", C.c_int, C.POINTER(DdcConfig), fp, C.POINTER(C.c_int32), C.POINTER(vp))
    sig("sdr_ddc_set_nco_step", C.c_int, vp, C.c_int, C.c_int)
    sig("sdr_ddc_process_device", C.c_int, vp, vp, C.c_size_t, vp, C.c_size_t)
    sig("sdr_ddc_process_host", C.c_int, vp, vp, C.c_size_t, vp, C.c_size_t)
    sig("sdr_ddc_nco_table", C.c_int, fp, fp)
    sig("sdr_chan_create", C.c_int, C.POINTER(ChanConfig), fp, C.POINTER(C.c_int32), C.POINTER(vp))
    sig("sdr_chan_process_device", C.c_int, vp, vp, C.c_size_t, vp, C.c_size_t)
    sig("sdr_chan_process_host", C.c_int, vp, vp, C.c_size_t, vp, C.c_size_t)
    sig("sdr_chan_tile_outputs", C.c_int, C.c_int, C.c_int, C.c_int)
    for obj in ("ddc", "chan"):
        sig(f"sdr_iq_{obj}_set_correction", C.c_int, vp, C.POINTER(IqCorrection))
        sig(f"sdr_iq_{obj}_enable_sums", C.c_int, vp, C.c_int)
        sig(f"sdr_iq_{obj}_read_sums", C.c_int, vp, C.POINTER(IqSums))
    sig("sdr_iq_correction_from_sums", C.c_int, C.POINTER(IqSums), C.c_int, C.POINTER(IqCorrection))
    sig("sdr_nb_create", C.c_int, C.POINTER(NbConfig), C.POINTER(vp))
    sig("sdr_nb_set_threshold", C.c_int, vp, C.c_int, C.c_int)
    sig("sdr_nb_process_device", C.c_int, vp, vp, C.c_size_t, vp)
    sig("sdr_nb_process_host", C.c_int, vp, vp, C.c_size_t, vp)
    sig("sdr_nb_read_stats", C.c_int, vp, C.POINTER(NbStats))
    sig("sdr_nb_tile_samples", C.c_int, C.c_int, C.c_int)
    sig("sdr_nb_blank_host", C.c_int, C.POINTER(NbConfig), vp, C.c_size_t, vp, C.POINTER(NbStats))
    sig("sdr_fine_create", C.c_int, C.POINTER(FineConfig), fp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(vp))
    sig("sdr_fine_set_nco_step", C.c_int, vp, C.c_int, C.c_int)
    sig("sdr_fine_set_input", C.c_int, vp, C.c_int, C.c_int)
    sig("sdr_fine_process_device", C.c_int, vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t)
    sig("sdr_fine_tune", C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32))
    sig("sdr_chain_create", C.c_int, C.POINTER(ChainConfig), C.POINTER(vp))
    sig("sdr_chain_destroy", C.c_int, vp)
    sig("sdr_chain_set_stream", C.c_int, vp, vp)
    sig("sdr_chain_sync", C.c_int, vp)
    sig("sdr_chain_push_host", C.c_int, vp, vp, C.c_size_t, ip)
    sig("sdr_chain_push_device", C.c_int, vp, vp, C.c_size_t, ip)
    sig("sdr_chain_read_narrow", C.c_int, vp, C.c_int, C.c_int64, C.c_int, fp)
    sig("sdr_chain_stats", C.c_int, vp, C.POINTER(ChainCounts))
    sig("sdr_chain_granule", C.c_int64, C.c_int, C.c_int)
    sig("sdr_chain_min_ring", C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int)
    _lib = L
    return L


def _check(rc: int):
    if rc != OK:
        raise SdrError(rc, load().sdr_last_error().decode(errors="replace"))


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _results_buffers(c: Config):
    """Record arrays big enough for any batch of a bank (or group) of config `c`, and the sdr_results pointing at them."""
    chunks = (c.max_batch_frames // CUMULATION_SIZE + 2) * c.n_bands
    listeners = max(c.max_listeners * c.n_bands, 1)
    bufs = {
        "chunks": np.zeros(chunks, CHUNK_RESULT_DTYPE),
        "peaks": np.zeros(chunks * c.max_peaks, PEAK_DTYPE),
        "listeners": np.zeros(listeners, LISTENER_RESULT_DTYPE),
        "edges": np.zeros(listeners * min(c.max_batch_frames, 8192), EDGE_DTYPE),
        "runes": np.zeros(listeners * 2048, np.uint32),
    }
    rune_frames = np.zeros(listeners * 2048, np.uint32)
    r = Results()
    r.struct_size = C.sizeof(Results)
    for k, a in bufs.items():
        setattr(r, k, a.ctypes.data)
        setattr(r, k + "_cap", len(a))
    r.rune_frames = rune_frames.ctypes.data
    return bufs, rune_frames, r


def _poll_rows(entry, handle, state: dict, columns: int, wait: bool, rows_cap):
    """sdr_poll_rows / sdr_group_poll_rows: (batch_index, ndarray[n_rows, columns]), or None where the call would block.
    The buffer grows to what the call asks for; with a fixed rows_cap (in rows) ERR_BAD_SIZE is raised instead, the rows
    needed in the exception's n_rows."""
    n, batch = C.c_int(), C.c_int64()
    cap = rows_cap if rows_cap is not None else state.get("cap", 0)
    for _ in range(2):
        buf = state.get("buf")
        if buf is None or buf.size < cap * columns:
            buf = state["buf"] = np.zeros(max(cap * columns, 1), np.float32)
        rc = entry(handle, buf.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n), C.byref(batch), int(wait))
        if rc == ERR_WOULD_BLOCK:
            return None
        if rc == ERR_BAD_SIZE and rows_cap is None:
            cap = state["cap"] = n.value
            continue
        break
    if rc != OK:
        try:
            _check(rc)
        except SdrError as e:
            e.n_rows = n.value
            raise
    return batch.value, buf[:n.value * columns].reshape(n.value, columns).copy()


def _poll_reports(entry, handle, state: dict, wait: bool, cap):
    """sdr_poll_reports / sdr_group_poll_reports: (batch_index, ndarray of REPORT_DTYPE), or None where the call would
    block.  The buffer grows to what the call asks for; with a fixed cap (in records) ERR_BAD_SIZE is raised instead, the
    records needed in the exception's n_out."""
    n, batch = C.c_int(), C.c_int64()
    want = cap if cap is not None else state.get("cap", 0)
    for _ in range(2):
        buf = state.get("buf")
        if buf is None or buf.size < want:
            buf = state["buf"] = np.zeros(max(want, 1), REPORT_DTYPE)
        rc = entry(handle, C.c_void_p(buf.ctypes.data), want, C.byref(n), C.byref(batch), int(wait))
        if rc == ERR_WOULD_BLOCK:
            return None
        if rc == ERR_BAD_SIZE and cap is None:
            want = state["cap"] = n.value
            continue
        break
    if rc != OK:
        try:
            _check(rc)
        except SdrError as e:
            e.n_out = n.value
            raise
    return batch.value, buf[:n.value].copy()


def _results_dict(r: Results, bufs: dict, rune_frames: np.ndarray, copy: bool) -> dict:
    out = {"batch_index": r.batch_index, "first_frame": r.first_frame, "n_frames": r.n_frames,
           "runes_dropped": r.runes_dropped, "edges_dropped": r.edges_dropped}
    for k, a in bufs.items():
        v = a[:getattr(r, "n_" + k)]
        out[k] = v.copy() if copy else v
    v = rune_frames[:r.n_runes]
    out["rune_frames"] = v.copy() if copy else v
    return out


class Bank:
    """A bank of n_bands receivers on one GPU (see include/sdrainer_hip.h)."""

    def __init__(self, sample_rate: int, block_size: int, n_bands: int = 1, edge_width: int | None = None,
                 peak_threshold: float = 15.0, signal_debounce: int = 1, max_listeners: int = 30,
                 max_batch_frames: int = 1024, max_peaks: int = 1024, find_peaks: bool = True, trace: bool = False,
                 device_id: int = 0, hop: int = 0):
        """hop: samples from one frame's start to the next (overlapped frames); 0 = block_size."""
        L = load()
        if edge_width is None:
            edge_width = 70 * block_size // 512  # the reference default (rx/receiver.go:25) scaled with N
        self.cfg = Config(C.sizeof(Config), n_bands, sample_rate, block_size, edge_width, peak_threshold,
                          signal_debounce, max_listeners, max_batch_frames, max_peaks, int(find_peaks), int(trace),
                          device_id, hop)
        self.n = block_size
        self.n_bands = n_bands
        h = C.c_void_p()
        _check(L.sdr_create(C.byref(self.cfg), C.byref(h)))
        self._h = h
        self._L = L

    @classmethod
    def _view(cls, handle: C.c_void_p, cfg: Config) -> "Bank":
        """A Bank over a bank owned by someone else (a Group member): close() leaves it alone."""
        self = cls.__new__(cls)
        self.cfg, self.n, self.n_bands = cfg, cfg.block_size, cfg.n_bands
        self._h, self._L, self._owner = handle, load(), False
        return self

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_owner", True):
                self._L.sdr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # producer ---------------------------------------------------------------------------------
    def set_stream(self, stream_ptr: int):
        _check(self._L.sdr_set_stream(self._h, C.c_void_p(stream_ptr)))

    def set_first_frame(self, frame: int):
        """sdr_set_first_frame: the bank's next frame gets this index (a multiple of CUMULATION_SIZE; a fresh bank only)."""
        _check(self._L.sdr_set_first_frame(self._h, int(frame)))

    def push_iq(self, band: int, sample_rate: int, iq: np.ndarray) -> int:
        """Returns the status code (0 ok) instead of raising for the reference's log-and-drop cases."""
        iq = np.ascontiguousarray(iq, dtype=np.float32)
        rc = self._L.sdr_push_iq(self._h, band, sample_rate, iq.ctypes.data_as(C.POINTER(C.c_float)), iq.size)
        if rc not in (OK, ERR_BAD_RATE, ERR_BAD_SIZE, ERR_WOULD_DROP, ERR_STATE):
            _check(rc)
        return rc

    def push_iq_sc16(self, band: int, sample_rate: int, iq: np.ndarray) -> int:
        """iq: int16 I,Q pairs (sc16); value = float32(x) / 32767.  Status code as push_iq."""
        iq = np.ascontiguousarray(iq, dtype=np.int16)
        rc = self._L.sdr_push_iq_sc16(self._h, band, sample_rate, iq.ctypes.data_as(C.POINTER(C.c_int16)), iq.size)
        if rc not in (OK, ERR_BAD_RATE, ERR_BAD_SIZE, ERR_WOULD_DROP, ERR_STATE):
            _check(rc)
        return rc

    def push_iq8(self, band: int, sample_rate: int, iq: np.ndarray, fmt: int) -> int:
        """iq: byte I,Q pairs, int8 for fmt = IQ8_CS8 (value x / 128) or uint8 for IQ8_CU8 (value (x - 127.5) / 128).  Status
        code as push_iq."""
        iq = _iq8_bytes(iq, fmt)
        rc = self._L.sdr_push_iq8(self._h, band, sample_rate, C.c_void_p(iq.ctypes.data), iq.size, fmt)
        if rc not in (OK, ERR_BAD_RATE, ERR_BAD_SIZE, ERR_WOULD_DROP, ERR_STATE):
            _check(rc)
        return rc

    def push_kiwi_snd(self, band: int, sample_rate: int, payload: bytes) -> int:
        """payload: body of one KiwiSDR SND message (17-byte header + big-endian int16 IQ)."""
        rc = self._L.sdr_push_kiwi_snd(self._h, band, sample_rate, payload, len(payload))
        if rc not in (OK, ERR_BAD_RATE, ERR_BAD_SIZE, ERR_WOULD_DROP, ERR_STATE):
            _check(rc)
        return rc

    def staged_frames(self, band: int) -> int:
        return self._L.sdr_staged_frames(self._h, band)

    def process_staged(self) -> int:
        n = C.c_int()
        _check(self._L.sdr_process_staged(self._h, C.byref(n)))
        return n.value

    def process_staged_limit(self, max_frames: int) -> int:
        n = C.c_int()
        _check(self._L.sdr_process_staged_limit(self._h, max_frames, C.byref(n)))
        return n.value

    def process_device(self, iq_dev_ptr: int, n_frames: int):
        _check(self._L.sdr_process_device(self._h, C.c_void_p(iq_dev_ptr), n_frames))

    def process_device_sc16(self, iq_dev_ptr: int, n_frames: int):
        """iq_dev_ptr: device memory [band][frame][2N] int16 (sc16), 16-byte aligned."""
        _check(self._L.sdr_process_device_sc16(self._h, C.c_void_p(iq_dev_ptr), n_frames))

    def process_device_iq8(self, iq_dev_ptr: int, n_frames: int, fmt: int):
        """iq_dev_ptr: device memory [band][frame][2N] bytes (cs8 or cu8 by fmt), 16-byte aligned."""
        _check(self._L.sdr_process_device_iq8(self._h, C.c_void_p(iq_dev_ptr), n_frames, fmt))

    @property
    def hop(self) -> int:
        """The effective hop: block_size unless the bank was created with a smaller one."""
        return self._L.sdr_hop(self._h)

    def process_device_stream(self, iq_dev_ptr: int, n_frames: int, band_stride_samples: int):
        """iq_dev_ptr: device memory, float32 I,Q; band b's frame f starts at sample b * band_stride_samples + f * hop."""
        _check(self._L.sdr_process_device_stream(self._h, C.c_void_p(iq_dev_ptr), n_frames, band_stride_samples))

    def process_device_stream_sc16(self, iq_dev_ptr: int, n_frames: int, band_stride_samples: int):
        """The same for int16 I,Q pairs (sc16)."""
        _check(self._L.sdr_process_device_stream_sc16(self._h, C.c_void_p(iq_dev_ptr), n_frames, band_stride_samples))

    def process_device_stream_iq8(self, iq_dev_ptr: int, n_frames: int, band_stride_samples: int, fmt: int):
        """The same for byte I,Q pairs (cs8 or cu8 by fmt); band_stride_samples a multiple of 8."""
        _check(self._L.sdr_process_device_stream_iq8(self._h, C.c_void_p(iq_dev_ptr), n_frames, band_stride_samples, fmt))

    def process_host(self, iq: np.ndarray) -> int:
        """iq: float32 [n_bands, n_frames, 2N] (or [n_frames, 2N] for one band) from host memory."""
        iq = np.ascontiguousarray(iq, dtype=np.float32).reshape(self.n_bands, -1, 2 * self.n)
        for b in range(self.n_bands):
            rc = self.push_iq(b, self.cfg.sample_rate, iq[b])
            if rc != OK:
                raise SdrError(rc, self._L.sdr_last_error().decode())
        return self.process_staged()

    def sync(self):
        _check(self._L.sdr_sync(self._h))

    # listeners --------------------------------------------------------------------------------
    def attach(self, band: int, bin_: int) -> int:
        lid = C.c_int()
        _check(self._L.sdr_attach(self._h, band, int(bin_), C.byref(lid)))
        return lid.value

    def attach_at(self, band: int, bin_: int, start_frame: int) -> int:
        """sdr_attach_at: a listener that listens from bank frame `start_frame` of the batch waiting for its listen half."""
        lid = C.c_int(-1)
        _check(self._L.sdr_attach_at(self._h, band, int(bin_), int(start_frame), C.byref(lid)))
        return lid.value

    def defer_listen(self, on: bool = True) -> None:
        _check(self._L.sdr_defer_listen(self._h, int(on)))

    @property
    def listen_pending(self) -> bool:
        return bool(self._L.sdr_listen_pending(self._h))

    def process_listen(self) -> None:
        _check(self._L.sdr_process_listen(self._h))

    def detach(self, band: int, lid: int):
        _check(self._L.sdr_detach(self._h, band, lid))

    def listener_count(self, band: int) -> int:
        return self._L.sdr_listener_count(self._h, band)

    def listener_stop(self, band: int, lid: int):
        _check(self._L.sdr_listener_stop(self._h, band, lid))

    # control ----------------------------------------------------------------------------------
    def set_peak_threshold(self, band: int, t: float):
        _check(self._L.sdr_set_peak_threshold(self._h, band, t))

    def set_edge_width(self, e: int):
        _check(self._L.sdr_set_edge_width(self._h, e))

    def set_signal_debounce(self, band: int, d: int):
        _check(self._L.sdr_set_signal_debounce(self._h, band, d))

    def set_center_frequency(self, band: int, f: int):
        _check(self._L.sdr_set_center_frequency(self._h, band, f))

    def set_find_peaks(self, on: bool):
        _check(self._L.sdr_set_find_peaks(self._h, int(on)))

    def set_window(self, w):
        """A window on the frames: block_size float32 values (copied), None removes it (sdr_set_window)."""
        _check(_set_window(self._L.sdr_set_window, self._h, w))

    # consumer ---------------------------------------------------------------------------------
    @property
    def last_batch_frames(self) -> int:
        return self._L.sdr_last_batch_frames(self._h)

    @property
    def total_frames(self) -> int:
        return self._L.sdr_total_frames(self._h)

    @property
    def last_batch_chunks(self) -> int:
        return self._L.sdr_last_batch_chunks(self._h)

    def read_peaks(self, band: int, chunk: int):
        cap = self.cfg.max_peaks
        arr = (Peak * cap)()
        n, fr = C.c_int(), C.c_int()
        _check(self._L.sdr_read_peaks(self._h, band, chunk, arr, cap, C.byref(n), C.byref(fr)))
        return [arr[i].astuple() for i in range(min(n.value, cap))], n.value, fr.value

    def read_cumulation(self, band: int, chunk: int) -> np.ndarray:
        out = np.empty(self.n, np.float32)
        _check(self._L.sdr_read_cumulation(self._h, band, chunk, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def read_text(self, band: int, lid: int) -> str:
        buf = C.create_string_buffer(16384)
        n = C.c_int()
        _check(self._L.sdr_read_text(self._h, band, lid, buf, len(buf), C.byref(n)))
        return buf.raw[:n.value].decode("utf-8")

    def read_edges(self, band: int, lid: int) -> np.ndarray:
        cap = min(self.cfg.max_batch_frames, 8192)
        out = np.zeros(cap, EDGE_DTYPE)
        n = C.c_int()
        _check(self._L.sdr_read_edges(self._h, band, lid, _vp(out), cap, C.byref(n)))
        return out[:min(n.value, cap)]

    def read_keying_bits(self, band: int, lid: int) -> np.ndarray:
        """Debounced on/off state per frame of the last batch, as uint8 [n_frames]."""
        nf = self.last_batch_frames
        words = (nf + 63) // 64
        out = np.zeros(max(words, 1), np.uint64)
        _check(self._L.sdr_read_keying_bits(self._h, band, lid, _vp(out), words))
        bits = np.unpackbits(out.view(np.uint8), bitorder="little")
        return bits[:nf].astype(np.uint8)

    def read_frame_records(self, band: int) -> np.ndarray:
        nf = self.last_batch_frames
        out = np.zeros(max(nf, 1), FRAME_REC_DTYPE)
        _check(self._L.sdr_read_frame_records(self._h, band, _vp(out), nf))
        return out[:nf]

    def read_trace(self, band: int, lid: int):
        nf = self.last_batch_frames
        v, r, d = np.zeros(nf, np.float32), np.zeros(nf, np.uint8), np.zeros(nf, np.uint8)
        _check(self._L.sdr_read_trace(self._h, band, lid, _vp(v), _vp(r), _vp(d), nf))
        return v, r, d

    def read_spectrum(self, band: int, frame: int):
        sp, psd = np.empty(self.n, np.float32), np.empty(self.n, np.float32)
        _check(self._L.sdr_read_spectrum(self._h, band, frame, _vp(sp), _vp(psd)))
        return sp, psd

    def read_decoder_state(self, band: int, lid: int) -> np.ndarray:
        out = np.empty(12)
        _check(self._L.sdr_read_decoder_state(self._h, band, lid, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    # graph mode -------------------------------------------------------------------------------
    @property
    def graph_batches(self) -> int:
        return self._L.sdr_graph_batches(self._h)

    def graph_capture(self, n_frames: int):
        _check(self._L.sdr_graph_capture(self._h, n_frames))

    def graph_launch(self, iq_dev_ptrs):
        arr = (C.c_void_p * len(iq_dev_ptrs))(*[C.c_void_p(int(p)) for p in iq_dev_ptrs])
        assert len(iq_dev_ptrs) == self.graph_batches
        _check(self._L.sdr_graph_launch(self._h, arr))

    def graph_capture_sc16(self, n_frames: int):
        _check(self._L.sdr_graph_capture_sc16(self._h, n_frames))

    def graph_launch_sc16(self, iq_dev_ptrs):
        arr = (C.c_void_p * len(iq_dev_ptrs))(*[C.c_void_p(int(p)) for p in iq_dev_ptrs])
        assert len(iq_dev_ptrs) == self.graph_batches
        _check(self._L.sdr_graph_launch_sc16(self._h, arr))

    def graph_capture_iq8(self, n_frames: int, fmt: int):
        _check(self._L.sdr_graph_capture_iq8(self._h, n_frames, fmt))

    def graph_launch_iq8(self, iq_dev_ptrs, fmt: int):
        arr = (C.c_void_p * len(iq_dev_ptrs))(*[C.c_void_p(int(p)) for p in iq_dev_ptrs])
        assert len(iq_dev_ptrs) == self.graph_batches
        _check(self._L.sdr_graph_launch_iq8(self._h, arr, fmt))

    def graph_release(self):
        _check(self._L.sdr_graph_release(self._h))

    # scope tap --------------------------------------------------------------------------------
    @property
    def scope_active(self) -> bool:
        return bool(self._L.sdr_scope_active(self._h))

    def scope_spectral_frame(self, band: int, chunk: int):
        """(header dict, Values float64[N]) of the "spectrum" scope stream for one completed cumulation."""
        fr = ScopeSpectralFrame()
        vals = np.empty(self.n, np.float64)
        _check(self._L.sdr_scope_read_spectral(self._h, band, chunk, C.byref(fr), vals.ctypes.data_as(C.POINTER(C.c_double)),
                                               self.n))
        hdr = {"frame": fr.frame, "from_frequency": fr.from_frequency, "to_frequency": fr.to_frequency,
               "signal_bin": fr.signal_bin, "threshold": fr.threshold, "n_values": fr.n_values}
        return hdr, vals

    def scope_demod_frames(self, band: int, lid: int) -> np.ndarray:
        """The listener's "demod" scope stream of the last batch: threshold, value, state, debounced per frame."""
        nf = self.last_batch_frames
        out = np.zeros(max(nf, 1), SCOPE_TIME_DTYPE)
        n = C.c_int()
        _check(self._L.sdr_scope_read_demod(self._h, band, lid, _vp(out), nf, C.byref(n)))
        return out[:min(nf, n.value)]

    def scope_decode_frames(self, band: int, lid: int) -> np.ndarray:
        """cw.Decoder's scope streams of the last batch (sdr_scope_decode_frame), one record per tick the listener took."""
        nf = self.last_batch_frames
        out = np.zeros(max(nf, 1), SCOPE_DECODE_DTYPE)
        n = C.c_int()
        _check(self._L.sdr_scope_read_decode(self._h, band, lid, _vp(out), nf, C.byref(n)))
        return out[:min(nf, n.value)]

    # bulk delivery ----------------------------------------------------------------------------
    def enable_results(self, on: bool = True):
        _check(self._L.sdr_enable_results(self._h, int(on)))
        if on and not hasattr(self, "_res"):
            self._res_bufs, self._rune_frames, self._res = _results_buffers(self.cfg)

    def enable_rows(self, columns: int):
        """sdr_enable_rows: one row of `columns` group maxima of the exact cumulation per completed cumulation (0: off)."""
        _check(self._L.sdr_enable_rows(self._h, int(columns)))
        if columns:
            self._rows_last = int(columns)  # (batches processed before rows were switched off keep their rows)

    @property
    def row_columns(self) -> int:
        return self._L.sdr_row_columns(self._h)

    def poll_rows(self, wait: bool = False, rows_cap: int | None = None):
        """sdr_poll_rows: (batch_index, ndarray[n_rows, columns]) of the oldest undelivered batch, which stays undelivered,
        or None.  Rows are in the order of that batch's chunks; nothing is divided by 100."""
        if not hasattr(self, "_rows_state"):
            self._rows_state = {}
        return _poll_rows(self._L.sdr_poll_rows, self._h, self._rows_state, getattr(self, "_rows_last", 0) or 1, wait, rows_cap)

    def enable_reports(self, on: bool = True):
        """sdr_enable_reports: one sdr_listener_report per active listener with every batch."""
        _check(self._L.sdr_enable_reports(self._h, int(on)))

    @property
    def reports_enabled(self) -> bool:
        return bool(self._L.sdr_reports_enabled(self._h))

    def poll_reports(self, wait: bool = False, cap: int | None = None):
        """sdr_poll_reports: (batch_index, ndarray of REPORT_DTYPE) of the oldest undelivered batch, which stays undelivered,
        or None.  Records are ordered by band, then listener id."""
        if not hasattr(self, "_reports_state"):
            self._reports_state = {}
        return _poll_reports(self._L.sdr_poll_reports, self._h, self._reports_state, wait, cap)

    def poll_peaks(self, wait: bool = True, copy: bool = True):
        """sdr_poll_peaks: chunks and peaks of the batch that waits for its listen half (it stays undelivered)."""
        return self.poll(wait, copy, _entry=self._L.sdr_poll_peaks)

    def poll(self, wait: bool = False, copy: bool = True, _entry=None):
        """Oldest finished batch as a dict of record arrays (views into reused buffers unless `copy`), or None."""
        r = self._res
        rc = (_entry or self._L.sdr_poll)(self._h, C.byref(r), int(wait))
        if rc == ERR_WOULD_BLOCK:
            return None
        _check(rc)
        return _results_dict(r, self._res_bufs, self._rune_frames, copy)

    def poll_counts(self, wait: bool = False):
        """Like poll() but returns only the record counts (the bench's timed loop: no Python-side copies)."""
        r = self._res
        rc = self._L.sdr_poll(self._h, C.byref(r), int(wait))
        if rc == ERR_WOULD_BLOCK:
            return None
        _check(rc)
        return (r.batch_index, r.n_chunks, r.n_peaks, r.n_listeners, r.n_edges, r.n_runes, r.runes_dropped, r.edges_dropped)

    @property
    def results_pending(self) -> int:
        return self._L.sdr_results_pending(self._h)

    def read_drop_counters(self):
        a, b = C.c_uint64(), C.c_uint64()
        _check(self._L.sdr_read_drop_counters(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    @staticmethod
    def runes_to_text(runes) -> str:
        return "".join(chr(int(x)) for x in runes)

    # measurement ------------------------------------------------------------------------------
    def profile_enable(self, on: bool):
        _check(self._L.sdr_profile_enable(self._h, int(on)))

    def profile_reset(self):
        _check(self._L.sdr_profile_reset(self._h))

    def profile_read(self) -> dict:
        out = {}
        for k, name in enumerate(KERNELS + (ROWS_KERNEL,) + REPORT_KERNELS):
            ms, n = C.c_double(), C.c_int()
            _check(self._L.sdr_profile_read(self._h, k, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out


class Group:
    """sdr_group: one bank per member device, driven as one bank of n_bands bands (band b on member b % n_members as
    local band b // n_members).  Per-band calls go through member(band)."""

    def __init__(self, device_ids, sample_rate: int, block_size: int, n_bands: int, edge_width: int | None = None,
                 peak_threshold: float = 15.0, signal_debounce: int = 1, max_listeners: int = 30,
                 max_batch_frames: int = 1024, max_peaks: int = 1024, find_peaks: bool = True, trace: bool = False,
                 hop: int = 0):
        """hop: passed on as sdr_config.hop; a group takes 0 or block_size only (ERR_BAD_ARG otherwise)."""
        L = load()
        if edge_width is None:
            edge_width = 70 * block_size // 512
        self.cfg = Config(C.sizeof(Config), n_bands, sample_rate, block_size, edge_width, peak_threshold,
                          signal_debounce, max_listeners, max_batch_frames, max_peaks, int(find_peaks), int(trace), 0, hop)
        self.n, self.n_bands, self.n_members = block_size, n_bands, len(device_ids)
        self.device_ids = list(device_ids)
        ids = (C.c_int32 * max(len(device_ids), 1))(*device_ids)
        h = C.c_void_p()
        _check(L.sdr_group_create(C.byref(self.cfg), ids, len(device_ids), C.byref(h)))
        self._h, self._L = h, L
        self._members = {}

    def close(self):
        if getattr(self, "_h", None):
            for m in self._members.values():  # (the views' banks go with the group)
                m._h = None
            self._L.sdr_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def member(self, band: int):
        """(Bank view of the member that holds `band`, local band index)."""
        bh, local = C.c_void_p(), C.c_int()
        _check(self._L.sdr_group_member(self._h, band, C.byref(bh), C.byref(local)))
        m = band % self.n_members
        if m not in self._members:
            c = Config.from_buffer_copy(self.cfg)
            c.n_bands = (self.n_bands - m + self.n_members - 1) // self.n_members
            c.device_id = self.device_ids[m]
            self._members[m] = Bank._view(bh, c)
        return self._members[m], local.value

    # producer ---------------------------------------------------------------------------------
    def push_iq(self, band: int, sample_rate: int, iq: np.ndarray) -> int:
        iq = np.ascontiguousarray(iq, dtype=np.float32)
        rc = self._L.sdr_group_push_iq(self._h, band, sample_rate, iq.ctypes.data_as(C.POINTER(C.c_float)), iq.size)
        if rc not in (OK, ERR_BAD_RATE, ERR_BAD_SIZE, ERR_WOULD_DROP, ERR_STATE):
            _check(rc)
        return rc

    def push_iq_sc16(self, band: int, sample_rate: int, iq: np.ndarray) -> int:
        iq = np.ascontiguousarray(iq, dtype=np.int16)
        rc = self._L.sdr_group_push_iq_sc16(self._h, band, sample_rate, iq.ctypes.data_as(C.POINTER(C.c_int16)), iq.size)
        if rc not in (OK, ERR_BAD_RATE, ERR_BAD_SIZE, ERR_WOULD_DROP, ERR_STATE):
            _check(rc)
        return rc

    def push_iq8(self, band: int, sample_rate: int, iq: np.ndarray, fmt: int) -> int:
        iq = _iq8_bytes(iq, fmt)
        rc = self._L.sdr_group_push_iq8(self._h, band, sample_rate, C.c_void_p(iq.ctypes.data), iq.size, fmt)
        if rc not in (OK, ERR_BAD_RATE, ERR_BAD_SIZE, ERR_WOULD_DROP, ERR_STATE):
            _check(rc)
        return rc

    def push_kiwi_snd(self, band: int, sample_rate: int, payload: bytes) -> int:
        rc = self._L.sdr_group_push_kiwi_snd(self._h, band, sample_rate, payload, len(payload))
        if rc not in (OK, ERR_BAD_RATE, ERR_BAD_SIZE, ERR_WOULD_DROP, ERR_STATE):
            _check(rc)
        return rc

    def process_staged(self) -> int:
        n = C.c_int()
        _check(self._L.sdr_group_process_staged(self._h, C.byref(n)))
        return n.value

    def process_staged_limit(self, max_frames: int) -> int:
        n = C.c_int()
        _check(self._L.sdr_group_process_staged_limit(self._h, max_frames, C.byref(n)))
        return n.value

    def process_device(self, iq_dev_ptrs, n_frames: int):
        """iq_dev_ptrs: one device pointer per member, each [local band][frame][2N] float32."""
        arr = (C.c_void_p * len(iq_dev_ptrs))(*[C.c_void_p(int(p)) for p in iq_dev_ptrs])
        _check(self._L.sdr_group_process_device(self._h, arr, n_frames))

    def process_device_sc16(self, iq_dev_ptrs, n_frames: int):
        """iq_dev_ptrs: one device pointer per member, each [local band][frame][2N] int16 (sc16)."""
        arr = (C.c_void_p * len(iq_dev_ptrs))(*[C.c_void_p(int(p)) for p in iq_dev_ptrs])
        _check(self._L.sdr_group_process_device_sc16(self._h, arr, n_frames))

    def process_device_iq8(self, iq_dev_ptrs, n_frames: int, fmt: int):
        """iq_dev_ptrs: one device pointer per member, each [local band][frame][2N] bytes (cs8 or cu8 by fmt)."""
        arr = (C.c_void_p * len(iq_dev_ptrs))(*[C.c_void_p(int(p)) for p in iq_dev_ptrs])
        _check(self._L.sdr_group_process_device_iq8(self._h, arr, n_frames, fmt))

    def sync(self):
        _check(self._L.sdr_group_sync(self._h))

    # control ----------------------------------------------------------------------------------
    def set_peak_threshold(self, band: int, t: float):
        _check(self._L.sdr_group_set_peak_threshold(self._h, band, t))

    def set_signal_debounce(self, band: int, d: int):
        _check(self._L.sdr_group_set_signal_debounce(self._h, band, d))

    def set_edge_width(self, e: int):
        _check(self._L.sdr_group_set_edge_width(self._h, e))

    def set_find_peaks(self, on: bool):
        _check(self._L.sdr_group_set_find_peaks(self._h, int(on)))

    def set_first_frame(self, frame: int):
        """sdr_group_set_first_frame: Bank.set_first_frame on every member."""
        _check(self._L.sdr_group_set_first_frame(self._h, int(frame)))

    def set_window(self, w):
        """sdr_group_set_window: the same window on every member, None removes it."""
        _check(_set_window(self._L.sdr_group_set_window, self._h, w))

    # delivery ---------------------------------------------------------------------------------
    def enable_results(self, on: bool = True):
        _check(self._L.sdr_group_enable_results(self._h, int(on)))
        if on and not hasattr(self, "_res"):
            self._res_bufs, self._rune_frames, self._res = _results_buffers(self.cfg)

    def poll(self, wait: bool = False, copy: bool = True, _entry=None):
        """Oldest batch every member has finished, merged (as Bank.poll), or None."""
        r = self._res
        rc = (_entry or self._L.sdr_group_poll)(self._h, C.byref(r), int(wait))
        if rc == ERR_WOULD_BLOCK:
            return None
        _check(rc)
        return _results_dict(r, self._res_bufs, self._rune_frames, copy)

    def poll_peaks(self, wait: bool = True, copy: bool = True):
        return self.poll(wait, copy, _entry=self._L.sdr_group_poll_peaks)

    def enable_rows(self, columns: int):
        """sdr_group_enable_rows: Bank.enable_rows on every member."""
        _check(self._L.sdr_group_enable_rows(self._h, int(columns)))
        self._row_columns = int(columns) or getattr(self, "_row_columns", 0)

    def poll_rows(self, wait: bool = False, rows_cap: int | None = None):
        """sdr_group_poll_rows: as Bank.poll_rows, the members' rows merged into the order of Group.poll's chunks."""
        if not hasattr(self, "_rows_state"):
            self._rows_state = {}
        return _poll_rows(self._L.sdr_group_poll_rows, self._h, self._rows_state, getattr(self, "_row_columns", 0) or 1, wait, rows_cap)

    def enable_reports(self, on: bool = True):
        """sdr_group_enable_reports: Bank.enable_reports on every member."""
        _check(self._L.sdr_group_enable_reports(self._h, int(on)))

    def poll_reports(self, wait: bool = False, cap: int | None = None):
        """sdr_group_poll_reports: as Bank.poll_reports, the members' records merged with global band numbers."""
        if not hasattr(self, "_reports_state"):
            self._reports_state = {}
        return _poll_reports(self._L.sdr_group_poll_reports, self._h, self._reports_state, wait, cap)

    def defer_listen(self, on: bool = True):
        _check(self._L.sdr_group_defer_listen(self._h, int(on)))

    def process_listen(self):
        _check(self._L.sdr_group_process_listen(self._h))

    def read_drop_counters(self):
        a, b = C.c_uint64(), C.c_uint64()
        _check(self._L.sdr_group_read_drop_counters(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value


def ddc_nco_table():
    """sdr_ddc_nco_table: (COS, SIN), float32 [DDC_NCO_SIZE] each - the table the down-converter mixes with.  Needs no GPU."""
    co, si = np.empty(DDC_NCO_SIZE, np.float32), np.empty(DDC_NCO_SIZE, np.float32)
    _check(load().sdr_ddc_nco_table(co.ctypes.data_as(C.POINTER(C.c_float)), si.ctypes.data_as(C.POINTER(C.c_float))))
    return co, si


def _raw_samples(samples, in_format: int) -> np.ndarray:
    """Raw samples of a DDC format as a C array: [n, 2] for a complex format, [n] for a real one."""
    dt = {DDC_F32: np.float32, DDC_SC16: np.int16, DDC_CS8: np.int8, DDC_CU8: np.uint8}[in_format & ~DDC_REAL]
    s = np.ascontiguousarray(samples, dt)
    if in_format & DDC_REAL:
        if s.ndim != 1:
            raise ValueError("a real in_format takes a one-dimensional array, one value per sample")
        return s
    return s.reshape(-1, 2)


class _Front:
    """What the front-end objects share (csrc/front.h): a handle of sdr_<object>_create on one stream, with a sample clock.
    A subclass names its entry points' prefix and sets _h and _L."""

    _prefix = ""  # "sdr_ddc", "sdr_chan", "sdr_fine", "sdr_nb"

    def _entry(self, name: str):
        return getattr(self._L, f"{self._prefix}_{name}")

    def close(self):
        if getattr(self, "_h", None):
            self._entry("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr: int):
        _check(self._entry("set_stream")(self._h, C.c_void_p(stream_ptr)))

    def set_first_sample(self, k0: int):
        """The next sample (of every input) gets index k0, >= 0 and a multiple of the decimation - the blanker: of block;
        before the first process call only."""
        _check(self._entry("set_first_sample")(self._h, int(k0)))

    @property
    def total_samples(self) -> int:
        return self._entry("total_samples")(self._h)

    def sync(self):
        _check(self._entry("sync")(self._h))


class _StageOne(_Front):
    """A down-converter or a channelizer: one wide raw stream in, from host memory too, with the IQ correction and the raw
    stream's sums (sdr_iq_<ddc|chan>_*)."""

    def _iq(self, name: str):
        return getattr(self._L, f"sdr_iq_{self._prefix[4:]}_{name}")

    def process_host(self, samples: np.ndarray, out_dev_ptr: int, band_stride_samples: int):
        """samples: the wide stream's raw samples in host memory, float32, int16, int8 or uint8 by in_format: [n, 2] for a
        complex format, [n] for a real one."""
        s = _raw_samples(samples, self.in_format)
        _check(self._entry("process_host")(self._h, C.c_void_p(s.ctypes.data), s.shape[0], C.c_void_p(out_dev_ptr), band_stride_samples))

    def set_iq_correction(self, c):
        """c: None (no correction), an IqCorrection or (dc_re, dc_im, gain_im, cross); from the next process call on."""
        _check(self._iq("set_correction")(self._h, _iq_correction(c)))

    def enable_iq_sums(self, on: bool = True):
        _check(self._iq("enable_sums")(self._h, int(bool(on))))

    def read_iq_sums(self) -> dict:
        """Waits for the stream; the sums since the last read as a dict of sdr_iq_sums' fields, and clears them."""
        s = IqSums()
        _check(self._iq("read_sums")(self._h, C.byref(s)))
        return s.asdict()


class Ddc(_StageOne):
    """sdr_ddc: one wide stream in, n_bands narrow float32 streams out in device memory (see include/sdrainer_hip.h).
    taps: the low-pass, float32, the same for every band; nco_steps: one step per band, the band's centre offset is
    step * input_rate / DDC_NCO_SIZE Hz."""

    _prefix = "sdr_ddc"

    def __init__(self, decimation: int, taps, nco_steps, in_format: int = DDC_F32, max_in_samples: int = 1 << 20,
                 device_id: int = 0):
        L = load()
        taps = np.ascontiguousarray(taps, np.float32).reshape(-1)
        steps = np.ascontiguousarray(nco_steps, np.int32).reshape(-1)
        self.cfg = DdcConfig(C.sizeof(DdcConfig), int(steps.size), decimation, int(taps.size), in_format, max_in_samples, device_id, 0)
        self.n_bands, self.decimation, self.n_taps, self.in_format = int(steps.size), decimation, int(taps.size), in_format
        h = C.c_void_p()
        _check(L.sdr_ddc_create(C.byref(self.cfg), taps.ctypes.data_as(C.POINTER(C.c_float)),
                                steps.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(h)))
        self._h, self._L = h, L

    def set_nco_step(self, band: int, step: int):
        _check(self._L.sdr_ddc_set_nco_step(self._h, band, int(step)))

    def process_device(self, in_dev_ptr: int, n_in_samples: int, out_dev_ptr: int, band_stride_samples: int):
        """Asynchronous on the DDC's stream: band b's n_in_samples / decimation outputs go to float32 I,Q sample
        b * band_stride_samples of out_dev_ptr on."""
        _check(self._L.sdr_ddc_process_device(self._h, C.c_void_p(in_dev_ptr), n_in_samples, C.c_void_p(out_dev_ptr), band_stride_samples))


def fine_tune(n_channels: int, decimation: int, target: int):
    """sdr_fine_tune: (channel, step) for a band centred `target` units of wide_rate / (65536 * decimation) from the wide
    stream's centre, behind a channelizer of n_channels channels with that decimation.  Exact in integers, needs no GPU.
    SdrError(ERR_BAD_ARG) for an illegal geometry or a target outside the wide stream."""
    ch, st = C.c_int32(), C.c_int32()
    _check(load().sdr_fine_tune(int(n_channels), int(decimation), int(target), C.byref(ch), C.byref(st)))
    return ch.value, st.value


class Fine(_Front):
    """sdr_fine: n_inputs float32 streams in device memory in (a channelizer's or a DDC's outputs), n_bands narrower float32
    streams out, each band tuned and decimated from the input it points at (see include/sdrainer_hip.h "fine converter").
    taps: the low-pass, the same for every band; nco_steps: one step per band, step * input_rate / DDC_NCO_SIZE Hz;
    inputs: the input each band reads (None: band b reads input b)."""

    _prefix = "sdr_fine"

    def __init__(self, n_inputs: int, decimation: int, taps, nco_steps, inputs=None, max_in_samples: int = 1 << 20,
                 device_id: int = 0):
        L = load()
        taps = np.ascontiguousarray(taps, np.float32).reshape(-1)
        steps = np.ascontiguousarray(nco_steps, np.int32).reshape(-1)
        ins = None if inputs is None else np.ascontiguousarray(inputs, np.int32).reshape(-1)
        if ins is not None and ins.size != steps.size:
            raise ValueError("one input index per band")
        self.cfg = FineConfig(C.sizeof(FineConfig), int(steps.size), n_inputs, decimation, int(taps.size), max_in_samples, device_id, 0)
        self.n_bands, self.n_inputs, self.decimation, self.n_taps = int(steps.size), n_inputs, decimation, int(taps.size)
        h = C.c_void_p()
        _check(L.sdr_fine_create(C.byref(self.cfg), taps.ctypes.data_as(C.POINTER(C.c_float)), steps.ctypes.data_as(C.POINTER(C.c_int32)),
                                 None if ins is None else ins.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(h)))
        self._h, self._L = h, L

    def set_nco_step(self, band: int, step: int):
        _check(self._L.sdr_fine_set_nco_step(self._h, band, int(step)))

    def set_input(self, band: int, input_: int):
        """Band `band` reads input `input_` from the next process call on (that input's history is on the device)."""
        _check(self._L.sdr_fine_set_input(self._h, band, int(input_)))

    def process_device(self, in_dev_ptr: int, in_stride_samples: int, n_in_samples: int, out_dev_ptr: int, band_stride_samples: int):
        """Asynchronous on the object's stream: input i's n_in_samples float32 I,Q samples are read from sample
        i * in_stride_samples of in_dev_ptr on, band b's n_in_samples / decimation outputs go to sample
        b * band_stride_samples of out_dev_ptr on.  The two ranges must not overlap."""
        _check(self._L.sdr_fine_process_device(self._h, C.c_void_p(in_dev_ptr), in_stride_samples, n_in_samples,
                                               C.c_void_p(out_dev_ptr), band_stride_samples))


def nb_tile_samples(in_format: int, block: int) -> int:
    """sdr_nb_tile_samples: the samples one workgroup of the blanker's gate kernel writes; negative for a format or block
    outside the limits.  Needs no GPU."""
    return load().sdr_nb_tile_samples(int(in_format), int(block))


def nb_blank_host(samples, in_format: int, block: int, window: int, ratio_q4: int, hold: int):
    """sdr_nb_blank_host: the blanker's definition over one whole stream from k = 0, on the host.  Needs no GPU.
    Returns (the blanked samples, shaped and typed as the input, and a dict of sdr_nb_stats' fields)."""
    s = _raw_samples(samples, in_format)
    out = np.empty_like(s)
    cfg = NbConfig(C.sizeof(NbConfig), int(in_format), int(block), int(window), int(ratio_q4), int(hold), int(block), 0)
    st = NbStats()
    _check(load().sdr_nb_blank_host(C.byref(cfg), C.c_void_p(s.ctypes.data), s.shape[0], C.c_void_p(out.ctypes.data), C.byref(st)))
    return out, st.asdict()


class Nb(_Front):
    """sdr_nb: the impulse noise blanker - raw samples in, raw samples of the same format out in device memory, in front of
    a Ddc, a Chan or the bank's raw-format calls (see include/sdrainer_hip.h)."""

    _prefix = "sdr_nb"

    def __init__(self, in_format: int, block: int, window: int, ratio_q4: int, hold: int, max_in_samples: int = 1 << 20,
                 device_id: int = 0):
        L = load()
        self.cfg = NbConfig(C.sizeof(NbConfig), in_format, block, window, ratio_q4, hold, max_in_samples, device_id)
        self.in_format, self.block, self.window = in_format, block, window
        h = C.c_void_p()
        _check(L.sdr_nb_create(C.byref(self.cfg), C.byref(h)))
        self._h, self._L = h, L

    def set_threshold(self, ratio_q4: int, hold: int):
        """From the next process call on; ratio_q4 = 0 switches judging off."""
        _check(self._L.sdr_nb_set_threshold(self._h, int(ratio_q4), int(hold)))

    def process_device(self, in_dev_ptr: int, n_in_samples: int, out_dev_ptr: int):
        """Asynchronous on the blanker's stream: n_in_samples raw samples from in_dev_ptr, blanked, to out_dev_ptr."""
        _check(self._L.sdr_nb_process_device(self._h, C.c_void_p(in_dev_ptr), n_in_samples, C.c_void_p(out_dev_ptr)))

    def process_host(self, samples: np.ndarray, out_dev_ptr: int):
        """samples: raw samples in host memory, int16, int8 or uint8 by in_format: [n, 2] complex, [n] real."""
        s = _raw_samples(samples, self.in_format)
        _check(self._L.sdr_nb_process_host(self._h, C.c_void_p(s.ctypes.data), s.shape[0], C.c_void_p(out_dev_ptr)))

    def read_stats(self) -> dict:
        """Waits for the stream; samples, impulses and blanked since the last read as a dict, and clears them."""
        s = NbStats()
        _check(self._L.sdr_nb_read_stats(self._h, C.byref(s)))
        return s.asdict()


def chan_tile_outputs(n_channels: int, decimation: int, n_taps: int) -> int:
    """sdr_chan_tile_outputs: the output times one workgroup of the channelizer's kernel computes; negative for a geometry
    outside the limits.  Needs no GPU."""
    return load().sdr_chan_tile_outputs(int(n_channels), int(decimation), int(n_taps))


class Chan(_StageOne):
    """sdr_chan: one wide stream in, the listed channels of an n_channels-band polyphase filter bank out as float32 streams in
    device memory (see include/sdrainer_hip.h).  taps: the prototype low-pass, float32, n_channels * P of them; channels: the
    channel of each output stream (None: all of them, 0 .. n_channels - 1).  Channel c is centred c * input_rate / n_channels
    above the wide stream's centre, (c - n_channels) * input_rate / n_channels for c >= n_channels / 2."""

    _prefix = "sdr_chan"

    def __init__(self, n_channels: int, decimation: int, taps, channels=None, in_format: int = DDC_F32,
                 max_in_samples: int = 1 << 20, device_id: int = 0):
        L = load()
        taps = np.ascontiguousarray(taps, np.float32).reshape(-1)
        chans = np.arange(n_channels, dtype=np.int32) if channels is None else np.ascontiguousarray(channels, np.int32).reshape(-1)
        self.cfg = ChanConfig(C.sizeof(ChanConfig), n_channels, decimation, int(taps.size), in_format, max_in_samples, device_id, int(chans.size))
        self.n_channels, self.decimation, self.n_taps, self.in_format = n_channels, decimation, int(taps.size), in_format
        self.channels = tuple(int(c) for c in chans)
        h = C.c_void_p()
        _check(L.sdr_chan_create(C.byref(self.cfg), taps.ctypes.data_as(C.POINTER(C.c_float)),
                                 chans.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(h)))
        self._h, self._L = h, L

    def process_device(self, in_dev_ptr: int, n_in_samples: int, out_dev_ptr: int, band_stride_samples: int):
        """Asynchronous on the channelizer's stream: output stream i's n_in_samples / decimation outputs go to float32 I,Q
        sample i * band_stride_samples of out_dev_ptr on."""
        _check(self._L.sdr_chan_process_device(self._h, C.c_void_p(in_dev_ptr), n_in_samples, C.c_void_p(out_dev_ptr), band_stride_samples))


def chain_granule(total_decimation: int, nb_block: int = 1) -> int:
    """sdr_chain_granule: G = lcm(2 * total_decimation, nb_block, 16); negative for an argument below 1.  Needs no GPU."""
    return load().sdr_chain_granule(int(total_decimation), int(nb_block))


def chain_min_ring(block_size: int, hop: int, piece: int, total_decimation: int) -> int:
    """sdr_chain_min_ring: 2 * block_size + piece / total_decimation rounded up to 4; negative for an illegal argument.
    Needs no GPU."""
    return load().sdr_chain_min_ring(int(block_size), int(hop), int(piece), int(total_decimation))


class Chain:
    """sdr_chain: [Nb] -> Ddc | Chan -> [Fine] -> Bank joined into one object that takes raw samples in pushes of any length
    and enqueues bank batches (see include/sdrainer_hip.h "receive chain").  The members are borrowed: they stay usable for
    their setters and for Bank.poll, and they outlive the chain.  ring_samples = 0 takes the minimum ring."""

    def __init__(self, bank: "Bank", ddc=None, chan=None, nb=None, fine=None, max_in_samples: int = 1 << 20, ring_samples: int = 0):
        L = load()
        self.members = (nb, ddc, chan, fine, bank)  # (kept alive as long as the chain is)
        stage = ddc if ddc is not None else chan
        self.in_format = stage.cfg.in_format if stage is not None else DDC_F32
        self.cfg = ChainConfig(C.sizeof(ChainConfig), max_in_samples, ring_samples, 0, *[m._h if m is not None else None for m in self.members])
        h = C.c_void_p()
        _check(L.sdr_chain_create(C.byref(self.cfg), C.byref(h)))
        self._h, self._L = h, L

    def close(self):
        if getattr(self, "_h", None):
            self._L.sdr_chain_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr: int):
        """The chain's stream and every member's."""
        _check(self._L.sdr_chain_set_stream(self._h, C.c_void_p(stream_ptr)))

    def sync(self):
        _check(self._L.sdr_chain_sync(self._h))

    def push_host(self, samples: np.ndarray) -> int:
        """samples: raw samples in host memory, typed by stage one's in_format, [n, 2] for a complex format and [n] for a real
        one; any n in 1 .. max_in_samples.  Returns the bank batches the push enqueued (Bank.poll delivers them)."""
        s = _raw_samples(samples, self.in_format)
        nb = C.c_int()
        _check(self._L.sdr_chain_push_host(self._h, C.c_void_p(s.ctypes.data), s.shape[0], C.byref(nb)))
        return nb.value

    def push_device(self, raw_dev_ptr: int, n_samples: int) -> int:
        """n_samples (a multiple of the granule) raw samples in device memory, 16-byte aligned, read in place."""
        nb = C.c_int()
        _check(self._L.sdr_chain_push_device(self._h, C.c_void_p(raw_dev_ptr), n_samples, C.byref(nb)))
        return nb.value

    def read_narrow(self, band: int, start: int, n: int) -> np.ndarray:
        """Narrow samples [start, start + n) of `band`, float32 [n, 2]; they must still be resident in the ring.  Waits for
        the stream."""
        out = np.empty((n, 2), np.float32)
        _check(self._L.sdr_chain_read_narrow(self._h, band, int(start), int(n), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def stats(self) -> dict:
        s = ChainCounts()
        _check(self._L.sdr_chain_stats(self._h, C.byref(s)))
        return s.asdict()


class AudioBank:
    """n_streams cw.AudioDemodulator instances (cw/audio.go) on the GPU."""

    def __init__(self, n_streams: int, pitch: float, sample_rate: int, max_blocks: int = 4096, device_id: int = 0):
        L = load()
        h = C.c_void_p()
        _check(L.sdr_audio_create(n_streams, pitch, sample_rate, max_blocks, device_id, C.byref(h)))
        self._h, self._L, self.n_streams = h, L, n_streams

    def close_handle(self):
        if getattr(self, "_h", None):
            self._L.sdr_audio_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close_handle()
        except Exception:
            pass

    @property
    def blocksize(self) -> int:
        return self._L.sdr_audio_blocksize(self._h)

    def set_scale(self, s: float):
        _check(self._L.sdr_audio_set_scale(self._h, s))

    def set_debounce(self, t: int):
        _check(self._L.sdr_audio_set_debounce(self._h, t))

    def set_magnitude_threshold(self, t: float):
        _check(self._L.sdr_audio_set_magnitude_threshold(self._h, t))

    def write(self, samples: np.ndarray):
        s = np.ascontiguousarray(samples, dtype=np.float32).reshape(self.n_streams, -1)
        _check(self._L.sdr_audio_write(self._h, s.ctypes.data_as(C.POINTER(C.c_float)), s.shape[1]))

    def close(self):
        _check(self._L.sdr_audio_close(self._h))

    def read_text(self, stream: int) -> str:
        buf = C.create_string_buffer(65536)
        n = C.c_int()
        _check(self._L.sdr_audio_read_text(self._h, stream, buf, len(buf), C.byref(n)))
        return buf.raw[:n.value].decode("utf-8")

    def read_trace(self, stream: int, max_blocks: int = 1 << 16):
        m, r, d = np.zeros(max_blocks), np.zeros(max_blocks, np.uint8), np.zeros(max_blocks, np.uint8)
        n = C.c_int()
        _check(self._L.sdr_audio_read_trace(self._h, stream, _vp(m), _vp(r), _vp(d), max_blocks, C.byref(n)))
        k = min(n.value, max_blocks)
        return m[:k], r[:k], d[:k]
