// sdr_device.h — HBM-resident state and launch geometry shared by the kernels and the C-ABI host code.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <mutex>

#include "../../include/sdrainer_hip.h"
#include "cw_decoder.h"
#include "fft_f64.h"
#include "host/batch_plan.h"
#include "host/overlap.h"

namespace sdr {

// Per-band state carried across batches (locals of Receiver.run, rx/receiver.go:339-346).
struct BandState {
    float nf_ring[SDR_NOISE_WINDOW];   // noiseFloorMean.values
    float dev_ring[SDR_NOISE_WINDOW];  // noiseDeviationMean.values
    float nf_sum, dev_sum;             // sumForMean of both
    int32_t next;                      // shared ring cursor (both means are Put once per frame)
    float peak_threshold;              // r.peakThreshold
};

// One listener of a band's pool (rx/listener.go:19-32 + cw/spectral.go:19-23).
struct ListenerSlot {
    int32_t active;
    int32_t bin;  // Peak.SignalBin
    cw::Debouncer deb;
    cw::DecoderState dec;
    uint32_t text_count;    // runes in the text buffer not yet read by the host
    uint32_t text_dropped;  // runes dropped because the buffer was full (since attach)
    // Bank frame index (32 bits, wrapping like every frame number on the device) from which the listener listens, and
    // from which the FFT kernel has tapped its bin (k_fft_psd.h "The tap").  Equal for a listener attached between
    // batches.  A listener bound to a batch whose spectra already exist (sdr_attach_at: strain-mode discovery without a
    // host round trip per cumulation) starts inside that batch - frames before start_frame do not reach its debouncer
    // or decoder - and reads its bin from the retained psd rows up to tapped_from.
    uint32_t start_frame;
    uint32_t tapped_from;
};

// Bank-wide overflow counters (device memory): what the reference's never-dropping io.Writer would have kept.
struct DropCounters {
    unsigned long long runes;  // decoded runes that found the listener's text buffer full
    unsigned long long edges;  // keying edges beyond a batch's per-listener edge buffer
};

// What k_find_peaks hands to the host, which finishes dsp.Peak (frequencies are float64 -> int).
struct DevPeak {
    int32_t from, to, signal_bin;
    float signal_value;
    float y1, y2, y3;  // cumulation at signal_bin-1, signal_bin, signal_bin+1 (PeakCenterCorrection)
};

struct NoiseGeom {
    int n;          // block size
    int edge;       // edgeWidth
    int window;     // windowSize = (N - 2 edge) / 10
    int n_windows;  // windows the reference's loop actually evaluates (9 or 10)
    double inv_n2;  // 1 / N^2 (exact power of two)
};

// What changes from batch to batch and would otherwise be a launch parameter.  In graph mode (sdr_graph_*) the
// launches of several batches are captured once and replayed, so these values live in device memory: the host
// writes the cursors of the batches of one replay into pinned memory and the graph's first node uploads them.
// A null cursor pointer means "use the launch parameters" (the eager path).
struct BatchCursor {
    const float *iq;      // this batch's input frames (float32 graphs)
    uint32_t frame_base;  // bank frame index of its first frame
    int32_t count0;       // cumulationCount before its first frame
    int32_t carry_in;     // which of the two carry buffers holds the cumulation carried in (0 / 1)
    int32_t reserved;
    const int16_t *iq_sc16;  // this batch's input frames (sc16 graphs: sdr_graph_capture_sc16)
    const uint8_t *iq8;      // this batch's input frames (cs8 / cu8 graphs: sdr_graph_capture_iq8)
};

struct ListenGeom {
    int n, stride, max_listeners, text_cap, edge_cap, bit_words, trace;
    uint32_t frame_base;
};

struct CumGeom {
    int n, stride, n_frames, count0, max_chunks;
};

// k_noise_scan.hip: one pass over a batch's psd for FindNoiseFloor's sums and the cumulations' bounds
struct ScanGeom {
    int n, edge, window, n_windows;          // NoiseGeom
    int stride, n_frames, count0, max_chunks;  // CumGeom
    int piece;                               // edge pieces hold at most this many bins (64 per-lane slots)
    int do_bound;                            // also the bound of every cumulation the batch completes
    int fpw;                                 // do_bound == 0: frames per workgroup (the slots play no part)
    int parts;                               // do_bound == 1: workgroups a slot's frames are dealt over (1 or 2)
};

struct PeakGeom {
    int n, stride, count0, max_chunks, max_peaks;
};

// Layout of one batch's block of pinned host memory (k_results.hip): byte offsets of its arrays
//   peak_counts [band][max_chunks][2] int32 (stored, found)   peaks [band][max_chunks][max_peaks] DevPeak
//   edge_counts [band][L] uint32                              edges [band][L][edge_cap] sdr_edge
//   text_counts [band][L] uint32                              text  [band][L][text_cap] uint32 runes
//                                                             text_frames [band][L][text_cap] uint32
//   drops       DropCounters of the bank as of this batch
struct ResultsLayout {
    int max_listeners, max_chunks, max_peaks, edge_cap, text_cap;
    size_t off_peak_counts, off_peaks, off_edge_counts, off_edges, off_text_counts, off_text, off_text_frames, off_drops, bytes;
};

// A stage's completion event can ride on the kernel's own dispatch packet (hipExtLaunchKernelGGL's stopEvent)
// instead of a hipEventRecord behind the kernel.  The record is a barrier packet of its own: the queue's next kernel
// waits for the command processor to retire it, which on the FFT queue was 27-36 us per batch with nothing running
// (0.200 ms per step for a 0.166 ms kernel launched back to back).  So where a launcher launches is a stream and,
// optionally, the event its work is done at: the scheduler's launchers take a LaunchAt where the others take a stream.
// The contract of every such launcher: given an event, it attaches it to the LAST kernel it launches and to no other
// (its earlier kernels get the plain stream).  One that returns hipSuccess without launching anything - launch_find_peaks
// at n_chunks == 0, the FFT launchers at n_frames <= 0 - leaves the event unrecorded: the caller must not ask for one there.
struct LaunchAt {
    hipStream_t stream;
    hipEvent_t done = nullptr;
    LaunchAt(hipStream_t s, hipEvent_t d = nullptr) : stream(s), done(d) {}  // (implicit: a plain stream is a launch without an event)
};
template <class F, class... A>
inline void launch_kernel(F kernel, dim3 grid, dim3 block, unsigned lds_bytes, LaunchAt at, A... args)
{
    if (at.done)
        hipExtLaunchKernelGGL(kernel, grid, block, lds_bytes, at.stream, nullptr, at.done, 0, args...);
    else
        hipLaunchKernelGGL(kernel, grid, block, lds_bytes, at.stream, args...);
}

// More than 64 KB of dynamic LDS needs the kernel attribute, which is per device: set it once on each device a bank
// launches on, for every kernel of one launcher.  `once` is that launcher's (a function-local static); the call that
// sets it returns what hipFuncSetAttribute said (the last failure), later calls on that device return hipSuccess.
struct LdsLimitOnce {
    static constexpr int kMaxDevices = 64;
    std::once_flag dev[kMaxDevices];
};
inline hipError_t raise_lds_limit_once(LdsLimitOnce &once, std::initializer_list<const void *> kernels, int bytes)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess)
        return e;
    if (dev < 0 || dev >= LdsLimitOnce::kMaxDevices)
        return hipErrorInvalidDevice;
    hipError_t attr_err = hipSuccess;
    std::call_once(once.dev[dev], [&] {
        for (const void *k : kernels) {
            const hipError_t ae = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
            if (ae != hipSuccess)
                attr_err = ae;
        }
    });
    return attr_err;
}

// The listeners' bins of every band and where their psd values go (k_fft_psd.h "The tap").
struct FftTap {
    const int32_t *bins;  // [band][stride], -1 = free slot
    float *out;           // [band][out_stride frames][stride]
    int n;                // slots in use (high-water mark over the bands); 0 = no tap
    int stride;           // max_listeners
    // k_fft_r32 only (null otherwise): psd at bin - 1, bin, bin + 1 of every slot, [band][out_stride frames][stride][4],
    // and the bins those rows were taken at, [band][stride] (-1 = none): what k_cum_refine reads instead of psd columns
    float *wide = nullptr;
    int32_t *used = nullptr;
};

// One FFT launch: what every FFT launcher takes.  `fft` names the kernel (host/batch_plan.h fft_kernel); launch_fft
// (fft_launch.hip) hands the launch to the unit that holds it, and a unit's entry refuses every kernel that is not its own.
struct FftLaunch {
    int logn;
    FftChoice fft;
    // samples of format fft.fmt (float32 pairs, sc16 words or cs8 / cu8 byte pairs); band b's frame f is the N samples from
    // sample b * in_stride + f * frame_stride on (host/overlap.h input_sample_offset; dense frames: frame_stride = N,
    // in_stride = n_frames * N; overlapped frames: frame_stride = hop < N, fft.strided)
    const void *iq;
    const BatchCursor *cur;
    const fft64::cplx *tw;  // the bank's twiddle buffer (build_twiddles); the k_fft_r32 units' entries take their own table
    float *psd;
    int n_frames, n_bands;
    size_t in_stride;
    int frame_stride, out_stride;
    FftTap tap;
    // k_fft_r32 only: its frame counters, [band][2] uint32, zero between launches (BatchSet::fft_ctr)
    uint32_t *steal = nullptr;
    // k_fft_2p only: one frame group's float64 intermediate, [band][FftChoice::group_frames][N] (BatchSet::fft_scratch)
    fft64::cplx *scratch = nullptr;
    // the bank's window table, [N] float32 in window_layout's order (sdr_set_window), null = none: sample i of every frame
    // is multiplied by its value in float32 before it is widened, by the windowed instances of the kernels (k_fft_psd.h,
    // k_fft_2p_a.h)
    const float *window = nullptr;
};

// fft_launch.hip: the one dispatch, a switch on fft_kernel(l.fft) over the units' entries below.  The bank's twiddle buffer
// for N = 16384 holds both kernels' tables, the 32-point kernel's behind the other: the k_fft_r32 units get theirs from here.
hipError_t launch_fft(const FftLaunch &l, LaunchAt at);
int twiddle_count(int logn);
void build_twiddles(int logn, const double *wre, const double *wim, fft64::cplx *out);
// The launchers are templates, instantiated by the kernel units (fft_input.h: InF32, InSc16, InIq8).  An instance launches
// the kernels of fft_kernel(l.fft) that are its own and returns hipErrorInvalidValue for any other id.
struct InF32;
struct InSc16;
struct InIq8;
// k_fft_psd.h, N = 512 - 16384, by input format and window: k_fft_psd.hip holds float32 and sc16 frames, k_fft_psd_win.hip
// the same with a window, k_fft_psd_iq8.hip 8-bit frames with a window and without
template <class IN, bool WIN>
hipError_t launch_fft_psd(const FftLaunch &l, LaunchAt at);
// fft_launch.hip: the order the windowed kernels read the window table in: out[N] from the caller's w[N] (sample order)
void window_layout(int logn, const float *w, float *out);
// k_fft_r32.h, one instance per k_fft_r32*.hip unit: N = 16384 as 512 threads x 32 points with the next frame prefetched
// into registers (l.tw: their own twiddle layout), dense frames (HOP = false) and frame_stride < N (a power of two; HOP =
// true).  Workgroups per band = max(1, ceil((CUs - fft.reserve_cus) / n_bands)), at most n_frames (unless
// fft.reserve_forced the reserve is at most CUs / kReserveDeviceShare)
template <class IN, bool HOP>
hipError_t launch_fft_r32(const FftLaunch &l, LaunchAt at);
// k_fft_2p_a.h, by input format, with a window or without: N = 32768 / 65536 as two phases over l.scratch (fft_2p.h), frame
// group by frame group.  k_fft_2p.hip holds F32 and SC16, k_fft_2p_iq8.hip CS8 and CU8; phase B of frames [f0, f0 + g) of a
// group is k_fft_2p.hip's for all of them
template <InFormat FMT>
hipError_t launch_fft_2p(const FftLaunch &l, LaunchAt at);
hipError_t launch_fft2p_b(const FftLaunch &l, int f0, int g, LaunchAt at);
// wpb_forced: windows per workgroup (0: the launcher's rule); mfma: the matrix-pipe variance kernel (host/batch_plan.h)
hipError_t launch_window_means(const float *psd, double *win_mean, NoiseGeom g, int n_frames, int n_bands, int stride, int wpb_forced,
                               LaunchAt at);
hipError_t launch_noise_stats(const float *psd, const double *win_mean, sdr_frame_rec *recs, NoiseGeom g, int n_frames,
                              int n_bands, int stride, bool mfma, LaunchAt at);
hipError_t launch_mfma_order_probe(unsigned *mismatches, int order, hipStream_t stream);  // k_noise.hip: sdr_self_check
hipError_t launch_thresholds(sdr_frame_rec *recs, BandState *st, int n_frames, int n_bands, int stride,
                             LaunchAt at);
hipError_t launch_listen_gather(const float *tap, const float *psd, const sdr_frame_rec *recs, const ListenerSlot *slots, const void *db_tab,
                                uint64_t *raw_bits, float *tr_values, uint8_t *tr_raw, const BatchCursor *cur, ListenGeom g, int n_frames,
                                int n_slots, int n_bands, LaunchAt at);
hipError_t launch_listen_decode(ListenerSlot *slots, const uint16_t *morse, const uint64_t *raw_bits,
                                uint64_t *deb_bits, uint32_t *text, uint32_t *text_frames, sdr_edge *edges,
                                uint32_t *edge_counts, uint8_t *tr_deb, DropCounters *drops, const BatchCursor *cur, ListenGeom g,
                                int n_frames, int n_bands, uint32_t *edge_pos, int pos_stride, LaunchAt at);
// k_report.hip (sdr_enable_reports): a slot's start and tap marks inside this batch, clamped to [0, n_frames], taken in front
// of the decoder; behind it one sdr_listener_report per slot (listener = -1: not active) into the batch's report block
hipError_t launch_report_marks(const ListenerSlot *slots, const BatchCursor *cur, ListenGeom g, int n_frames, int n_bands, int32_t *marks,
                               hipStream_t stream);
hipError_t launch_listen_report(const float *tap, const float *psd, const sdr_frame_rec *recs, const ListenerSlot *slots, const void *db_tab,
                                const uint64_t *deb_bits, const int32_t *marks, ListenGeom g, int n_frames, int n_slots, int n_bands,
                                sdr_listener_report *out, hipStream_t stream);
hipError_t launch_listener_stop(ListenerSlot *slot, const uint16_t *morse, uint32_t *text, uint32_t *text_frames, int text_cap,
                                uint32_t frame, DropCounters *drops, hipStream_t stream);
hipError_t launch_set_debounce(ListenerSlot *slots, int n, int threshold, hipStream_t stream);
// bound: the completed cumulations are bounded (else every slot exact); bound_done: k_psd_scan has written their unit counts
// in `parts` partial rows (slot 0's without the carry: it is added here, on the stream the carry is produced on)
hipError_t launch_cumulate(const float *psd, const void *db_tab, float *carry0, float *carry1, int carry_in, float *cum_out,
                           const float *cum_part, const BatchCursor *cur, CumGeom g, int n_slots, int n_bands, bool bound, bool bound_done,
                           int parts, LaunchAt at);
// k_noise_scan.hip: the FindNoiseFloor fields of every frame's record, certified or literal, and (do_bound) the unit counts
// of the completed cumulations, a slot's frames dealt over `parts` workgroups - one kernel
hipError_t launch_psd_scan(const float *psd, sdr_frame_rec *recs, float *cum_out, float *cum_part, const BatchCursor *cur, NoiseGeom ng,
                           CumGeom cg, int n_slots, int n_bands, bool do_bound, int parts, int force_exact, LaunchAt at);
hipError_t launch_noise_exact_check(const float *psd_band, sdr_frame_rec *recs_band, NoiseGeom ng, int n_frames, unsigned *mismatches,
                                    hipStream_t stream);
hipError_t launch_spectrum_row(const float *psd_row, float *out, int n, hipStream_t stream);
hipError_t launch_pack_listen(ListenerSlot *slots, const sdr_edge *edges, const uint32_t *edge_counts, const uint32_t *text,
                              const uint32_t *text_frames, const DropCounters *drops, ResultsLayout lay, int n_slots, int n_bands, unsigned char *host,
                              LaunchAt at);
hipError_t launch_pack_peaks(const DevPeak *peaks, const int *counts, const BatchCursor *cur, ResultsLayout lay, int find_peaks,
                             int n_frames, int n_chunks, int n_bands, unsigned char *host, LaunchAt at);
// cumulations a batch of n_frames completes when it starts at cumulationCount count0
__host__ __device__ inline int chunks_completed(int count0, int n_frames)
{
    const int first_len = SDR_CUMULATION_SIZE - count0;
    return n_frames >= first_len ? 1 + (n_frames - first_len) / SDR_CUMULATION_SIZE : 0;
}
hipError_t launch_unpack_be16(const uint8_t *raw, float *out, size_t n_values, hipStream_t stream);
hipError_t launch_unpack_sc16(const int16_t *raw, float *out, size_t n_values, hipStream_t stream);  // little-endian int16 values
hipError_t launch_unpack_iq8(const uint8_t *raw, float *out, size_t n_values, bool cu8, hipStream_t stream);  // cs8 / cu8 bytes (iq8.h)
hipError_t launch_find_peaks(float *cum, const float *psd, const void *db_tab, const float *carry0, const float *carry1, int carry_in,
                             const sdr_frame_rec *recs, DevPeak *peaks, int *counts, const BatchCursor *cur, PeakGeom g, int n_frames,
                             int n_chunks, int n_bands, Refine refine, FftTap tap, LaunchAt at);  // tap: .wide / .used / .n / .stride of this batch's FFT (or null)
// k_cum_rows: every cumulation the batch completes, exact and reduced to `columns` group maxima, into the row block
hipError_t launch_cum_rows(const float *psd, const void *db_tab, const float *carry0, const float *carry1, int carry_in, const BatchCursor *cur,
                           CumGeom g, int columns, int n_chunks, int n_bands, float *rows, hipStream_t stream);
hipError_t launch_cumulation_row(const float *psd_band, const void *db_tab, const float *carry_in_band, float *row_out, CumGeom g, int slot,
                                 hipStream_t stream);

}  // namespace sdr
