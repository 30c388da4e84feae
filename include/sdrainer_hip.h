/*
 * sdrainer_hip.h — C ABI of libsdrainer_hip.so, the MI355X (gfx950) implementation of sdrainer's
 * per-block IQ-strainer DSP.  This is the drop-in boundary: plain pointers and sizes, no C++ or
 * framework types.  A Go maintainer binds it with cgo behind rx.Receiver / rx.Listener
 * (INTEGRATION.md shows the stub); this repo's C++ host mirror (sdrainer_amd/csrc/host/) and its
 * Python tests bind exactly the same symbols.
 *
 * One `sdr_bank` = n_bands independent receivers of identical geometry (sample rate, block size) on
 * one GPU and one HIP stream.  A band is what the reference calls a Receiver: it owns its rolling
 * noise floor, cumulation, listeners and decoders and shares nothing with other bands
 * (rx/receiver.go:64-91), which is what makes bands shardable across GPUs.
 *
 * Reference interface each entry point replaces (paths relative to the reference checkout):
 *   sdr_create / sdr_destroy        rx.NewReceiver + Receiver.Start / Stop      rx/receiver.go:93,130,148
 *   sdr_push_iq                     Receiver.IQData(sampleRate, []float32)      rx/receiver.go:315-334
 *   sdr_process_staged              the frame case of Receiver.run              rx/receiver.go:353-463
 *   sdr_process_device              same, for IQ already resident in HBM (the "IQ ring buffer")
 *   sdr_attach / sdr_detach         ListenerPool.BindNext + Listener.Attach / Detach + Release
 *                                                                               rx/listener.go:84-108,214-248
 *   sdr_set_peak_threshold          Receiver.SetPeakThreshold                   rx/receiver.go:208-212
 *   sdr_set_edge_width              Receiver.SetEdgeWidth                       rx/receiver.go:214-218
 *   sdr_set_signal_debounce         Receiver.SetSignalDebounce                  rx/receiver.go:238-244
 *   sdr_set_center_frequency        Receiver.SetCenterFrequency                 rx/receiver.go:246-253
 *   sdr_read_peaks                  the []dsp.Peak of dsp.FindPeaks             dsp/fft.go:179-188,254-285
 *   sdr_read_text                   the io.Writer each Listener's Decoder writes to  cw/decode.go:352-355
 *   sdr_read_edges / _trace         what cw.SpectralDemodulator.Tick hands to Decoder.Tick  cw/spectral.go:48-54
 *   sdr_read_frame_records          locals of Receiver.run (noise floor, thresholds)  rx/receiver.go:381-385
 *   sdr_push_kiwi_snd               decodeIQMessage + kiwi.Process.IQData       kiwi/client.go:284-308, kiwi/kiwi.go:94-105
 *   sdr_push_iq_sc16, *_sc16        Receiver.IQData fed by decodeIQBytes' complex int16 samples  kiwi/client.go:298-308
 *   sdr_push_iq8, *_iq8             Receiver.IQData fed by an 8-bit receiver's bytes (cs8 / cu8), widened on the device
 *   sdr_audio_*                     cw.AudioDemodulator (Goertzel audio path)   cw/audio.go:37-211
 *   sdr_enable_results / sdr_poll   the consumer side in bulk: what Receiver.run hands to its listeners'
 *                                   io.Writer (rx/receiver.go:123, ChannelWriter :508-539) and to the
 *                                   Reporter (rx/rx.go:11-17), one call per processed batch
 *   sdr_defer_listen / sdr_poll_peaks / sdr_attach_at / sdr_process_listen
 *                                   the discovery branch of Receiver.run - FindPeaks at a cumulation boundary,
 *                                   PeaksTable.FindNext, ListenerPool.BindNext, Listener.Attach, the listener
 *                                   hearing the next frame - without one host round trip per cumulation
 *                                                                               rx/receiver.go:404-426
 *   sdr_scope_*                     scope.Scope.ShowSpectralFrame / ShowTimeFrame  scope/scope.go:14-37,
 *                                   call sites rx/receiver.go:428-457, cw/spectral.go:56-81, cw/decode.go:228-243
 *
 * Semantics kept from the reference: setters take effect between frames, never mid-frame (here: at
 * the next process call, rx/receiver.go:166-172); wrong sample rate / block size / a full queue do
 * not abort anything, the call returns a status the shim maps to the reference's log-and-drop
 * (rx/receiver.go:319-333).  Two semantic extensions: batching - a process call consumes many frames per band, in
 * order - and overlapped frames (sdr_config.hop): frame f of a band is the block_size samples from sample f * hop of
 * the band's stream on, so the spectral resolution stays sample_rate / block_size while a decoder tick lasts
 * hop / sample_rate.  Receiver.IQData takes one explicit frame per call and does not care whether consecutive frames
 * share samples: every frame still produces what the reference produces for its block_size samples, and only what
 * means TIME follows the hop (the listeners' cw.NewDecoder(sampleRate, hop)).
 *
 * Threading: a bank is single-producer (like the reference's run goroutine, all DSP state is owned
 * by one thread); different banks are independent.  One more thread may consume: sdr_poll and
 * sdr_results_pending may be called from a thread of their own while the producer thread processes (the
 * reference's Reporter callbacks arrive on other goroutines too).
 */
#ifndef SDRAINER_HIP_H
#define SDRAINER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDR_ABI_VERSION 2

/* status codes */
#define SDR_OK 0
#define SDR_ERR_BAD_ARG 1    /* null pointer, index out of range, unsupported geometry            */
#define SDR_ERR_BAD_RATE 2   /* wrong incoming sample rate  -> reference logs + drops (:319-322)  */
#define SDR_ERR_BAD_SIZE 3   /* wrong incoming block size   -> reference logs + drops (:323-326)  */
#define SDR_ERR_WOULD_DROP 4 /* staging queue full          -> reference logs + drops (:328-333)  */
#define SDR_ERR_HIP 5        /* a HIP runtime call failed; sdr_last_error() has the text          */
#define SDR_ERR_NO_SLOT 6    /* listener pool exhausted (rx/listener.go:214-217)                  */
#define SDR_ERR_STATE 7      /* call not valid in the current state                               */
#define SDR_ERR_WOULD_BLOCK 8 /* sdr_poll: no finished batch is waiting to be delivered                */

/* rx/receiver.go:15-27 */
#define SDR_CUMULATION_SIZE 100
#define SDR_NOISE_WINDOW 60
#define SDR_DBM_SHIFT 120
#define SDR_DEFAULT_PEAK_THRESHOLD 15.0f
#define SDR_DEFAULT_EDGE_WIDTH 70
#define SDR_DEFAULT_LISTENER_POOL_SIZE 30

typedef struct sdr_bank sdr_bank;

typedef struct sdr_config {
    int32_t struct_size;      /* = sizeof(sdr_config), ABI guard                                  */
    int32_t n_bands;          /* independent receivers in this bank                               */
    int32_t sample_rate;      /* Receiver.Start(sampleRate, blockSize)                            */
    int32_t block_size;       /* complex samples per frame; power of two in [512, 65536]          */
    int32_t edge_width;       /* bins ignored at both spectrum edges (default 70)                 */
    float peak_threshold;     /* dB over the noise floor for the peak scan (default 15)           */
    int32_t signal_debounce;  /* BoolDebouncer threshold of new listeners (default 1)             */
    int32_t max_listeners;    /* listener pool size per band (reference: 30 strain / 1 decode)    */
    int32_t max_batch_frames; /* capacity: frames per band per process call                       */
    int32_t max_peaks;        /* capacity: peaks reported per completed cumulation                */
    int32_t find_peaks;       /* 1: run FindPeaks on every completed 100-frame cumulation         */
    int32_t trace;            /* 1: keep per-frame value / raw / debounced traces (parity, scope) */
    int32_t device_id;        /* HIP device ordinal                                               */
    int32_t hop;              /* samples from one frame's start to the next.  0 = block_size: frames do not overlap
                               * (a zeroed field, the word was reserved before, is exactly the behaviour before it
                               * existed).  Else a power of two, block_size / 16 <= hop <= block_size, hop >= 32;
                               * anything else: SDR_ERR_BAD_ARG from sdr_create                                     */
} sdr_config;

/* dsp.Peak[float32,int] (dsp/fft.go:179-188), fixed-width */
typedef struct sdr_peak {
    int32_t from, to;
    int64_t from_frequency, to_frequency, signal_frequency;
    float signal_value;
    int32_t signal_bin;
} sdr_peak;

/* per-frame locals of Receiver.run (rx/receiver.go:381-385,394) */
typedef struct sdr_frame_rec {
    float min_mean;    /* FindNoiseFloor: T(minValue)                      */
    float dev_in;      /* value put into noiseDeviationMean                */
    double variance;   /* FindNoiseFloor: variance (consumed only through dev_in: see sdr_read_frame_records) */
    float nf_in;       /* value put into noiseFloorMean                    */
    float noise_dev;   /* noiseDeviation                                   */
    float noise_floor; /* noiseFloor                                       */
    float peak_thr;    /* peakThreshold = r.peakThreshold + noiseFloor     */
    float listen_thr;  /* noiseFloor + noiseDeviation (Listener.Listen)    */
    float pad;
} sdr_frame_rec;

/* Frame numbering.  A bank counts its frames in 64 bits: sdr_total_frames, sdr_results.first_frame, sdr_chunk_result.frame
 * and the scope frames are int64 bank frame indices (0 for the first frame of a new bank, or what sdr_set_first_frame
 * gave it).  The two 32-bit fields, sdr_edge.frame and sdr_results.rune_frames, hold the bank frame index MODULO 2^32 (a
 * record per keying edge has no room for more, and on the device frames are only ever compared as differences).  A
 * consumer widens one against the first_frame of the batch that delivered it:
 *     frame = first_frame + (int32_t)(f32 - (uint32_t)first_frame)
 * (csrc/host/delivery.h widen_frame; exact while the frame lies within 2^31 of first_frame, and an edge or a rune lies in
 * its batch or, a flushed rune, right before it). */

/* one keying edge of a listener: debounced state changed at this frame (the bank frame index modulo 2^32, see above) */
typedef struct sdr_edge {
    uint32_t frame;
    uint32_t state; /* 1 = key down */
} sdr_edge;

const char *sdr_last_error(void);
int sdr_abi_version(void);

/* lifecycle ---------------------------------------------------------------------------------- */
int sdr_create(const sdr_config *cfg, sdr_bank **out);
int sdr_destroy(sdr_bank *bank);
/* The effective hop in samples: cfg->hop, or block_size where that was 0. */
int sdr_hop(sdr_bank *bank);
/* Checks, on device `device_id`, the one piece of UNDOCUMENTED hardware behaviour a code path of the library depends on:
 * that the float64 matrix instruction the ORDERED variance chains of FindNoiseFloor can run on (dsp/fft.go:244-249: `sum +=
 * term`, one rounding per step; csrc/k_noise.hip) adds its four terms one after the other, each step rounded, in order -
 * 1024 wide-range quadruples against the same chains on the vector ALU, bit for bit.  0 = as assumed.  Since round 5 the
 * default noise-floor path (csrc/k_noise_scan.hip: values certified where they are consumed, literal loops on the vector
 * ALU for the rest) does not use that instruction, and sdr_create runs the check - once per device and process, refusing
 * to create a bank (SDR_ERR_HIP, message in sdr_last_error) where it fails - only when the environment selects the
 * ordered chains (SDR_NOISE_PATH=chains).  A host has no need to call it; one that does should do so AFTER its first
 * sdr_create: the probe launches a kernel, and HIP deals its four hardware queues to streams as they come - work issued
 * before a bank's streams exist can leave two of them sharing a queue (measured: graph mode at two thirds of its rate).
 * The caller's current device is left as it was. */
int sdr_self_check(int device_id);
/* Run on this hipStream_t (NULL = the null stream).  Must be called before the first process call
 * or while the bank is idle. */
int sdr_set_stream(sdr_bank *bank, void *hip_stream);
/* The bank's next frame gets the index `frame`: a host that restarts a bank inside a running stream keeps its frame
 * numbering and, with it, the stream clock (sdr_total_frames returns `frame` at once; every first_frame, chunk frame,
 * scope frame, edge frame and rune frame that follows counts from it, and sdr_attach_at takes start frames counted so).
 * Nothing else changes: batch_index starts at 0 and cumulations complete at frames = 99 (mod SDR_CUMULATION_SIZE) as in
 * any bank, which is why `frame` must be a multiple of SDR_CUMULATION_SIZE.
 *   SDR_ERR_BAD_ARG: frame < 0, or not a multiple of SDR_CUMULATION_SIZE.
 *   SDR_ERR_STATE: the bank has processed a frame, has input staged (sdr_push_*), holds or has held a listener, or has
 *     a graph captured: call it right after sdr_create.
 * sdr_group_set_first_frame (declared with the group): the same frame on every member, or on none (a member that refuses
 * leaves the others as they were). */
int sdr_set_first_frame(sdr_bank *bank, int64_t frame);

/* producer side ------------------------------------------------------------------------------ */
/* Copies n_floats/(2*block_size) interleaved I,Q float32 frames of `band` from host memory into the
 * bank's pinned staging queue (the input is borrowed only for the duration of the call).
 * On a bank with hop < block_size the band's input is one continuous stream, pushed in pieces of any whole number of
 * hops (n_floats a multiple of 2 * hop; SDR_ERR_BAD_SIZE otherwise - at hop == block_size that is the rule above).  The
 * staging set holds (max_batch_frames - 1) * hop + block_size samples per band, of which block_size - hop are the
 * history a batch leaves for the next one; a push that would exceed it is SDR_ERR_WOULD_DROP. */
int sdr_push_iq(sdr_bank *bank, int band, int sample_rate, const float *iq, size_t n_floats);
/* KiwiSDR source: `payload` is one "SND" websocket message body (kiwi/client.go:284-308): a 17-byte
 * header (flags, sequence number, S-meter, GPS) followed by big-endian int16 I,Q pairs.  The raw bytes
 * are staged and unpacked ON THE DEVICE to float32 = float32(int16) / 32767 when the batch is processed;
 * like kiwi.Process.IQData (kiwi/kiwi.go:94-105) the message must hold whole frames (BAD_SIZE
 * otherwise).  A band's batch must not mix this with sdr_push_iq (SDR_ERR_STATE).  Not offered with overlapped frames
 * yet: SDR_ERR_STATE on a bank with hop < block_size. */
int sdr_push_kiwi_snd(sdr_bank *bank, int band, int sample_rate, const uint8_t *payload, size_t n_bytes);
/* Complete frames currently staged for `band`: max(0, (history + staged - (block_size - hop)) / hop) samples-wise, where
 * history is the block_size - hop samples kept from the previous batch (0 before the first; always 0 at hop == block_size). */
int sdr_staged_frames(sdr_bank *bank, int band);
/* Uploads and processes min-over-bands staged frames; *n_frames_out = frames consumed per band.  With overlapped
 * frames only the samples pushed since the last batch are uploaded (hop / block_size of the bytes the frames hold); the
 * last block_size - hop samples of the consumed frames stay on the device as the next batch's history. */
int sdr_process_staged(sdr_bank *bank, int *n_frames_out);
/* Same, but at most max_frames per band (lets a host stop at a cumulation boundary, where the
 * reference attaches a new listener: rx/receiver.go:409-426). */
int sdr_process_staged_limit(sdr_bank *bank, int max_frames, int *n_frames_out);
/* Processes n_frames per band of IQ already in device memory, layout [band][frame][block_size][2]
 * float32 (band stride = n_frames*2*block_size floats), 16-byte aligned (SDR_ERR_BAD_ARG otherwise).
 * Asynchronous on the bank's stream.  On a bank with hop < block_size this layout has no meaning: SDR_ERR_STATE (use
 * sdr_process_device_stream). */
int sdr_process_device(sdr_bank *bank, const float *iq_dev, int n_frames);
/* Device-resident streams, the input of overlapped frames: band b's frame f is the block_size complex samples starting at
 * sample b * band_stride_samples + f * hop of iq_dev.  The caller guarantees (n_frames - 1) * hop + block_size readable
 * samples per band; band_stride_samples is at least that and a multiple of 4 samples, iq_dev 16-byte aligned
 * (SDR_ERR_BAD_ARG otherwise).  Two bands may read one buffer at different offsets.  Continuity between calls is the ring
 * owner's business: the next call's pointer is n_frames * hop samples further on.  With hop == block_size and
 * band_stride_samples == n_frames * block_size the call is sdr_process_device, bit for bit.  _sc16: int16 I,Q pairs as
 * sdr_process_device_sc16.  Asynchronous on the bank's stream. */
int sdr_process_device_stream(sdr_bank *bank, const float *iq_dev, int n_frames, size_t band_stride_samples);
int sdr_process_device_stream_sc16(sdr_bank *bank, const int16_t *iq_dev, int n_frames, size_t band_stride_samples);
/* Complex int16 input ("sc16": int16 I, then int16 Q, little-endian), the format of IQ sources and capture hardware.  A
 * sample's value is float32(x) / 32767, correctly rounded (kiwi/client.go:298-308): every result is bit-identical to the
 * float32 calls fed with those values.  n_values counts int16 values (2 per sample); statuses are the float32 calls'.
 *   sdr_push_iq_sc16: as sdr_push_iq; the int16 values are staged and uploaded as they are (half the bytes) and converted
 *     on the device.  A band's batch must not mix it with sdr_push_iq or sdr_push_kiwi_snd (SDR_ERR_STATE).
 *   sdr_process_device_sc16: as sdr_process_device, layout [band][frame][block_size][2] int16, 16-byte aligned; the FFT
 *     kernels read the int16 values themselves (no float32 copy). */
int sdr_push_iq_sc16(sdr_bank *bank, int band, int sample_rate, const int16_t *iq, size_t n_values);
int sdr_process_device_sc16(sdr_bank *bank, const int16_t *iq_dev, int n_frames);
/* Complex 8-bit input: one byte I, then one byte Q per sample, the format of the common wide-band receivers.  `format`:
 *   SDR_IQ8_CS8  signed bytes (HackRF class):     value = float32(x) / 128
 *   SDR_IQ8_CU8  unsigned bytes (RTL-SDR class):  value = (float32(x) - 127.5) / 128 = (2 x - 255) / 256
 * Both are exact in float32 for all 256 inputs, so nothing is rounded and every result is bit-identical to the float32
 * calls fed with those values - with a window (the operand is the converted value), with a hop, in a graph replay and
 * through a group.  A caller who wants another convention (a measured DC offset such as 127.4, division by 127) converts
 * to float32 itself and uses the float32 calls.  n_values counts bytes (2 per sample); statuses are the sc16 calls'; any
 * other `format` is SDR_ERR_BAD_ARG.
 *   sdr_push_iq8: as sdr_push_iq_sc16 (whole hops; only the new samples are uploaded): the bytes are staged and uploaded as
 *     they are (a quarter of float32's bytes) and converted on the device.  A band's batch must not mix kinds - float32,
 *     KiwiSDR, sc16, cs8, cu8 (SDR_ERR_STATE).
 *   sdr_process_device_iq8: as sdr_process_device, layout [band][frame][block_size][2] bytes, 16-byte aligned; the FFT
 *     kernels read the bytes themselves (no float32 copy).  SDR_ERR_STATE on a bank with hop < block_size.
 *   sdr_process_device_stream_iq8: as sdr_process_device_stream_sc16, band_stride_samples a multiple of 8 samples (16
 *     bytes). */
#define SDR_IQ8_CS8 0
#define SDR_IQ8_CU8 1
int sdr_push_iq8(sdr_bank *bank, int band, int sample_rate, const void *iq, size_t n_values, int format);
int sdr_process_device_iq8(sdr_bank *bank, const void *iq_dev, int n_frames, int format);
int sdr_process_device_stream_iq8(sdr_bank *bank, const void *iq_dev, int n_frames, size_t band_stride_samples, int format);
/* Blocks until everything queued on the bank's stream has finished. */
int sdr_sync(sdr_bank *bank);

/* per-signal entry --------------------------------------------------------------------------- */
/* Binds a fresh listener (new debouncer + new decoder, Reset) to spectrum bin `bin` of `band`,
 * effective from the next processed frame. */
int sdr_attach(sdr_bank *bank, int band, int bin, int *listener_id);
int sdr_detach(sdr_bank *bank, int band, int listener_id);
int sdr_listener_count(sdr_bank *bank, int band);
/* Flush the listener's pending character (cw.Decoder.stop, cw/decode.go:352-354). */
int sdr_listener_stop(sdr_bank *bank, int band, int listener_id);

/* control ------------------------------------------------------------------------------------ */
/* The reference applies each control between two frames (Receiver.do, rx/receiver.go:217-253); the bank applies it between
 * two batches: a call takes effect from the next batch enqueued (the next replay of a captured graph) and leaves every
 * batch enqueued before it - finished or not - as it was, what the read calls hand out of the last one included.
 *   sdr_set_peak_threshold   the band's threshold in dB over the noise floor, from the next batch's first frame on - the
 *                            cumulation that completes behind the call is searched with the new value, as in the
 *                            reference.  Any float (+Inf: no peak).  Accepted with a listen half pending (it reaches the
 *                            batch behind the pending one) and with a graph captured.  Drains the bank.
 *   sdr_set_edge_width       FindNoiseFloor's edge width, the whole bank's, from the next batch on; SDR_ERR_BAD_ARG if
 *                            negative or if fewer than 10 bins are left.  Accepted with a listen half pending.  With a
 *                            graph captured a different value invalidates the capture (sdr_graph_launch returns
 *                            SDR_ERR_STATE: release, capture again); the value the capture has leaves it valid.
 *                            sdr_read_frame_records of the batch before the call still reads with the width it ran with.
 *   sdr_set_signal_debounce  the debounce threshold of the band's listeners attached at the call (dsp/dsp.go:154-156: the
 *                            threshold and nothing else of the debouncer - below 2 it passes the raw state through and
 *                            keeps its count and states as they were, and a later threshold >= 2 picks them up again).  A
 *                            listener attached later starts from sdr_config.signal_debounce.  SDR_ERR_STATE while a
 *                            listen half is pending (sdr_process_listen first): its frames lie before the call.
 *                            Accepted with a graph captured (the next replay runs with it).
 *   sdr_set_find_peaks       whether completed cumulations are searched, from the next batch on (a cumulation that is
 *                            not searched is delivered with no peaks).  Accepted with a listen half pending; with a graph
 *                            captured a different value invalidates the capture.
 * A band out of range is SDR_ERR_BAD_ARG and changes nothing. */
int sdr_set_peak_threshold(sdr_bank *bank, int band, float threshold);
int sdr_set_edge_width(sdr_bank *bank, int edge_width);
int sdr_set_signal_debounce(sdr_bank *bank, int band, int debounce);
int sdr_set_center_frequency(sdr_bank *bank, int band, int64_t frequency);
int sdr_set_find_peaks(sdr_bank *bank, int on);
/* A window on the frames (the third semantic extension).  window[i] multiplies sample i of every
 * frame of every band before the transform: re' = float32(re * window[i]), im' = float32(im * window[i]), one correctly
 * rounded float32 multiplication each; for sc16 input the operand is the converted value, so sc16 stays bit-identical to
 * float32 input holding those values.  Everything behind the multiplication is the reference's arithmetic on those
 * float32 values: the results equal the reference fed with frames multiplied so.  The FFT kernels multiply while they
 * read the input, for every input path (host pushes, KiwiSDR payloads, device frames and streams), with any hop.
 *   window: host pointer to n == block_size float32 values, copied (borrowed for the call only).  NULL with n == 0
 *     removes the window; a bank that never had one, or had it removed, runs the kernels it ran without this call.
 *   Takes effect from the first frame of the next process call; batches already enqueued keep the window they were
 *     enqueued with (the call drains the bank: it is a rare control call, not one for the sample path).
 *   SDR_ERR_BAD_ARG: n != block_size, or a null table with n != 0.  SDR_ERR_STATE: the listen half of a deferred batch is
 *     pending, or a graph is captured (set the window, then capture: the capture records it and replays with it).
 * Nothing is normalised: absolute levels fall by the window's gains - a periodic Hann window takes 6.02 dB off a carrier
 * (coherent gain 0.5) and 4.26 dB off noise (power gain 0.375).  Thresholds are relative to the measured noise floor and
 * need no change; a caller who wants calibrated levels scales the table (Hann: by 2 for carriers).
 * N = 16384: k_fft_r32 has no windowed form, a windowed bank runs the 16-point kernel at every batch length. */
int sdr_set_window(sdr_bank *bank, const float *window, int n);

/* consumer side (all synchronise with the stream first) --------------------------------------- */
/* Frames per band consumed by the last process call / since bank creation. */
int sdr_last_batch_frames(sdr_bank *bank);
int64_t sdr_total_frames(sdr_bank *bank);
/* Number of 100-frame cumulations completed by the last process call. */
int sdr_last_batch_chunks(sdr_bank *bank);
/* Peaks of completed cumulation `chunk` (0-based within the last batch).  *frame_in_batch = index
 * of the frame that completed it.  *n_out = the runs FindPeaks found, which may exceed what was stored: the first
 * min(*n_out, max_peaks, max) records of `out` are filled, in bin order (the peaks_found of sdr_chunk_result). */
int sdr_read_peaks(sdr_bank *bank, int band, int chunk, sdr_peak *out, int max, int *n_out, int *frame_in_batch);
/* Cumulated spectrum (sum over 100 frames, float32[block_size]) of that chunk (rx/receiver.go:404-407), every bin the
 * reference's ordered float32 sum.  The pipeline itself keeps a cumulation exact only where FindPeaks reads it; this call
 * recomputes the whole row from the batch's retained spectra and the carry it started from. */
int sdr_read_cumulation(sdr_bank *bank, int band, int chunk, float *out);
/* Decoded text of a listener since the last read, UTF-8 (what the reference writes to io.Writer). */
int sdr_read_text(sdr_bank *bank, int band, int listener_id, char *out, int max_bytes, int *n_bytes);
/* Keying edges of a listener produced by the last process call.  *n_out = the edges of the batch, which may exceed the
 * min(max_batch_frames, 8192) a batch stores per listener: the first min(*n_out, that capacity, max) records of `out` are
 * filled, the rest are counted in edges_dropped.  The decoder takes every edge whatever was stored. */
int sdr_read_edges(sdr_bank *bank, int band, int listener_id, sdr_edge *out, int max, int *n_out);
/* Packed debounced on/off bits of the last batch: bit (f & 63) of word (f >> 6). */
int sdr_read_keying_bits(sdr_bank *bank, int band, int listener_id, uint64_t *out, int max_words);
/* The last batch's frame records.  min_mean, dev_in, nf_in and everything behind them are the reference's bits on the hot
 * path already (certified from order-free sums, or the literal loops: csrc/noise_cert.h); `variance`, which nothing
 * downstream reads as a float64, is recomputed here by the reference's ordered loop, and the certified fields are checked
 * against the literal ones on the way (SDR_ERR_STATE on a difference: a defect, never seen). */
int sdr_read_frame_records(sdr_bank *bank, int band, sdr_frame_rec *out, int max);
/* trace == 1 only: per-frame value handed to Listen, raw and debounced state of a listener. */
int sdr_read_trace(sdr_bank *bank, int band, int listener_id, float *values, uint8_t *raw, uint8_t *debounced, int max);
/* spectrum (dB+120, fftshifted) and psd of frame `frame` of the last batch, float32[block_size] each. */
int sdr_read_spectrum(sdr_bank *bank, int band, int frame, float *spectrum, float *psd);
/* cw.Decoder state of a listener: ticks, onStart, offStart, wpm, on{low,high,last,thr}, off{...}. */
int sdr_read_decoder_state(sdr_bank *bank, int band, int listener_id, double *out12);

/* bulk delivery ----------------------------------------------------------------------------- */
/* With results enabled every process call ends with two small kernels that copy what the batch produced - peaks
 * of each completed cumulation, each listener's keying edges and newly decoded runes - into pinned host memory;
 * sdr_poll hands the oldest finished batch to the caller WITHOUT draining the pipeline (it looks at two events)
 * and never loses one: a batch whose buffers are about to be reused is parked on the host first.  Text is then
 * delivered here only (sdr_read_text finds nothing left).  Decoded runes the device could not store and edges
 * beyond a batch's edge buffer are counted, never silently lost: runes_dropped / edges_dropped (both stay 0
 * while every batch is polled; the reference's io.Writer never drops). */
typedef struct sdr_chunk_result {
    int32_t band;
    int32_t n_peaks;    /* peaks[first_peak .. first_peak + n_peaks) */
    int64_t frame;      /* frame (counted from bank start) that completed this 100-frame cumulation */
    int32_t first_peak;
    int32_t peaks_found; /* runs FindPeaks found; > n_peaks only if max_peaks was too small */
} sdr_chunk_result;

typedef struct sdr_listener_result {
    int32_t band, listener;
    int32_t first_edge, n_edges; /* edges[first_edge ..): frame counted from bank start, state 1 = key down */
    int32_t first_rune, n_runes; /* runes[first_rune ..): Unicode code points in decode order */
} sdr_listener_result;

typedef struct sdr_results {
    int32_t struct_size;   /* = sizeof(sdr_results), ABI guard (in) */
    int32_t n_frames;      /* frames per band in this batch (out) */
    int64_t batch_index;   /* 0-based count of process calls (out) */
    int64_t first_frame;   /* bank frame index of the batch's first frame (out) */
    /* caller-owned buffers with their capacities in records (in); counts written (out).  If a buffer is too
     * small the call returns SDR_ERR_BAD_SIZE with the n_* fields set to what is needed and delivers nothing. */
    sdr_chunk_result *chunks;
    int32_t chunks_cap, n_chunks;
    sdr_peak *peaks;
    int32_t peaks_cap, n_peaks;
    sdr_listener_result *listeners; /* listeners with at least one edge or rune in this batch */
    int32_t listeners_cap, n_listeners;
    sdr_edge *edges;
    int32_t edges_cap, n_edges;
    uint32_t *runes;       /* Unicode code points */
    uint32_t *rune_frames; /* same capacity and count as runes: bank frame index of the Tick that wrote each rune */
    int32_t runes_cap, n_runes;
    uint64_t runes_dropped, edges_dropped; /* since bank creation (out) */
} sdr_results;

int sdr_enable_results(sdr_bank *bank, int on);
/* Oldest finished, undelivered batch -> *r.  SDR_ERR_WOULD_BLOCK if there is none (yet); with wait != 0 the
 * call blocks until the oldest undelivered batch has finished (WOULD_BLOCK only if nothing was processed). */
int sdr_poll(sdr_bank *bank, sdr_results *r, int wait);

/* Waterfall rows: the exact spectrum of every completed cumulation, reduced, travelling with its batch (what the reference
 * hands to scope.ShowSpectralFrame once per cumulation, rx/receiver.go:428-457, for a display of a few hundred to a few
 * thousand columns - without a bank created with trace = 1, without a synchronising read, and for every batch).
 *   sdr_enable_rows(columns): 0 switches rows off (a new bank's state: it launches exactly the kernels it launched before
 *     this call existed); else a power of two, 64 <= columns <= block_size (anything else: SDR_ERR_BAD_ARG).  From the next
 *     process call on, a kernel behind the batch's cumulations forms every bin's exact cumulation - what
 *     sdr_read_cumulation returns: the reference's ordered float32 sum of the 100 spectra, fft-shifted - and packs one row
 *     of `columns` float32 values per completed cumulation beside the batch's peaks.  With G = block_size / columns,
 *         row[j] = the result of  m = cum[j*G]; for k in 1 .. G-1: v = cum[j*G + k]; if (v > m) m = v;
 *     a group whose first bin is NaN gives NaN, any other the maximum of its non-NaN values; G = 1 is the cumulation itself.
 *     NOTHING IS DIVIDED BY 100: the values are sums over SDR_CUMULATION_SIZE frames of dB + SDR_DBM_SHIFT, the caller scales
 *     (the reference shows cumulation / 100).  Needs sdr_enable_results (SDR_ERR_STATE without; switching results off
 *     switches rows off); SDR_ERR_STATE while a listen half is pending.  Like sdr_enable_results it invalidates a captured
 *     graph (sdr_graph_launch returns SDR_ERR_STATE until the next capture; a capture made with rows on records the rows
 *     kernel).  The first call, and a call with another non-zero column count, allocates pinned memory and drains the bank;
 *     the latter needs every batch delivered first (SDR_ERR_STATE otherwise).
 *   sdr_row_columns: the current setting.
 *   sdr_poll_rows: a peek, like sdr_poll_peaks: copies the rows of the oldest finished, undelivered batch - the batch the
 *     next sdr_poll hands out, which stays undelivered - to `rows` (rows_cap counts rows of `columns` values) and sets
 *     *batch_index.  Row i belongs to chunks[i] of that batch's sdr_results: by band, then chunk.  It waits for the device
 *     exactly where sdr_poll would (wait != 0) and returns SDR_ERR_WOULD_BLOCK where sdr_poll would; SDR_ERR_BAD_SIZE with
 *     *n_rows set to the rows needed and nothing copied if rows_cap is too small; SDR_OK with *n_rows = 0 for a batch that
 *     completed no cumulation or was processed with rows off.  A batch parked on the host (a ring set about to be reused,
 *     graph replays, sdr_graph_release) keeps its rows.  With the listen half deferred the rows belong to the spectral
 *     half: sdr_poll_rows sees the waiting batch as soon as sdr_poll_peaks does.  One consumer thread, as for sdr_poll. */
int sdr_enable_rows(sdr_bank *bank, int columns);
int sdr_row_columns(sdr_bank *bank);
int sdr_poll_rows(sdr_bank *bank, float *rows, int rows_cap, int *n_rows, int64_t *batch_index, int wait);

/* Listener reports: how strong every listened signal was in a batch, and how fast it is keyed - the "dB over noise, WPM"
 * of a skimmer's spot line - travelling with the batch, without a bank created with trace = 1 and without a
 * synchronising read per listener.
 * With reports on, every batch delivers one sdr_listener_report for each listener slot that was active in the batch's
 * listen stage, ordered by band, then listener id.  For such a listener the ticks f run over the frames of the batch that
 * reach it (from start_frame on for a listener bound with sdr_attach_at, every frame otherwise; a listener whose
 * start_frame lies behind the batch reports ticks = 0).  Per tick
 *     v[f]  = the float32 value the gather compares with the frame's threshold, dB + SDR_DBM_SHIFT (Listener.Listen's value),
 *     d[f]  = the DEBOUNCED bit, what the decoder sees,
 *     nf[f] = sdr_frame_rec.noise_floor of the frame;
 * a tick is MEASURED if neither v[f] nor nf[f] is NaN.  Values are quantised to 1/256 dB,
 *     q(x) = (int32) rint(clamp(x, -1024, 1024) * 256)
 * in float32 with round-half-to-even (the product is exact; +-Inf clamps).  Every field but wpm is an integer function of
 * exact float32 values and sums and maxima of integers have no order: any kernel schedule gives the same bits, and the
 * reports of consecutive batches add up (sums and counts add, on_max_q takes the maximum, wpm the last value) - any cut of
 * a stream into batches gives the same totals.  That is why the record holds fixed-point sums and not float means.
 * The caller's SNR is (on_sum_q - floor_sum_q) / (256.0 * ticks_on): the mean key-down level over the band's noise floor
 * in dB.  Nothing is divided on the device.  A band of zero samples clamps at q = -262144 (v and nf are -Inf). */
typedef struct sdr_listener_report {      /* 64 bytes */
    int32_t band, listener, bin;
    int32_t ticks;        /* frames of this batch that reached the listener                      */
    int32_t ticks_on;     /* measured ticks with d = 1                                           */
    int32_t ticks_off;    /* measured ticks with d = 0   (ticks - on - off: unmeasured, NaN)     */
    int32_t on_max_q;     /* max q(v) over the ticks_on ticks; INT32_MIN if there are none       */
    int32_t reserved;     /* 0 */
    int64_t on_sum_q;     /* sum q(v)  over the ticks_on ticks                                   */
    int64_t off_sum_q;    /* sum q(v)  over the ticks_off ticks                                  */
    int64_t floor_sum_q;  /* sum q(nf) over the ticks_on ticks                                   */
    double  wpm;          /* Decoder.wpm behind the batch's last tick (out12[3] of sdr_read_decoder_state) */
} sdr_listener_report;
/*   sdr_enable_reports(on): off in a new bank (it launches exactly the kernels it launched before this call existed).
 *     Needs sdr_enable_results (SDR_ERR_STATE without; switching results off switches reports off); SDR_ERR_STATE while a
 *     listen half is pending.  The first call that switches reports on allocates pinned memory (n_bands * max_listeners
 *     records per buffer set) and drains the bank.  It invalidates a captured graph (sdr_graph_launch returns SDR_ERR_STATE
 *     until the next capture; a capture made with reports on records the report kernels).
 *   sdr_reports_enabled: the current setting.
 *   sdr_poll_reports: a peek at the batch the next sdr_poll hands out, which stays undelivered: its records to `out` (cap
 *     counts records), *n_out and *batch_index set.  It waits for the device and returns SDR_ERR_WOULD_BLOCK exactly where
 *     sdr_poll would: the reports belong to the listen half, so a batch whose listen half is deferred shows them only
 *     after sdr_process_listen.  SDR_ERR_BAD_SIZE with *n_out set to the records needed and nothing copied if cap is too
 *     small; SDR_OK with *n_out = 0 for a batch processed with reports off or without an active listener.  A batch parked
 *     on the host keeps its reports.  One consumer thread, as for sdr_poll. */
int sdr_enable_reports(sdr_bank *bank, int on);
int sdr_reports_enabled(sdr_bank *bank);
int sdr_poll_reports(sdr_bank *bank, sdr_listener_report *out, int cap, int *n_out, int64_t *batch_index, int wait);

/* Strain-mode discovery over a long batch (rx/receiver.go:404-426: one listener bound per completed cumulation, to a
 * peak of that cumulation, listening from the very next frame).  With deferral on (needs sdr_enable_results), a
 * sdr_process_* call runs the spectral half of the batch only - FFT, noise floor, thresholds, cumulations and FindPeaks
 * of EVERY cumulation the batch completes - and the bank refuses further batches until sdr_process_listen has run the
 * listeners over the retained spectra.  In between the host reads the peaks (sdr_poll_peaks: the chunks / peaks part of
 * sdr_results, the batch stays undelivered; sdr_poll delivers it whole once the listen half has run) and binds listeners
 * with sdr_attach_at: like sdr_attach, but the listener listens from bank frame `start_frame` on (counted from the
 * bank's first frame; between the first frame of the waiting batch and the next frame to be processed).  Frames before
 * start_frame never reach its debouncer or decoder, so it produces exactly what a listener attached there frame by frame
 * would have.  Neither call waits for the device. */
int sdr_defer_listen(sdr_bank *bank, int on);
int sdr_listen_pending(sdr_bank *bank);
int sdr_poll_peaks(sdr_bank *bank, sdr_results *results, int wait);
int sdr_attach_at(sdr_bank *bank, int band, int bin, int64_t start_frame, int *listener_id);
int sdr_process_listen(sdr_bank *bank);
/* Batches processed but not yet delivered. */
int sdr_results_pending(sdr_bank *bank);
/* Overflow counters without bulk delivery (synchronises): runes the decoders could not store because a text
 * buffer was full, and keying edges beyond the edge buffer of the batches so far. */
int sdr_read_drop_counters(sdr_bank *bank, uint64_t *runes_dropped, uint64_t *edges_dropped);

/* graph mode --------------------------------------------------------------------------------- */
/* The steady state of Receiver.run (rx/receiver.go:353-463) for sdr_graph_batches() consecutive batches of
 * n_frames frames each, recorded once and replayed: one kernel-only hipGraph per stream of the bank (two on the peaks
 * stream), ordered inside a replay by events around whole graphs, with up to four replays in flight over buffer sets of
 * their own (allocated at capture), so that consecutive replays overlap stage by stage like consecutive eager batches.
 * Needs a bank on a real stream (sdr_set_stream with a non-null stream) and, once captured, all processing to go
 * through sdr_graph_launch (sdr_process_* return SDR_ERR_STATE until sdr_graph_release).  Attaching or detaching a
 * listener, sdr_enable_results, sdr_enable_rows, sdr_enable_reports, sdr_set_find_peaks and sdr_set_edge_width with a
 * value other than the capture's invalidate the capture (sdr_graph_launch returns SDR_ERR_STATE:
 * capture again).  Results are read / polled exactly as after sdr_process_device;
 * the "last batch" of the read calls is the last replay's last.  Not offered with overlapped frames yet:
 * sdr_graph_capture(_sc16, _iq8) on a bank with hop < block_size returns SDR_ERR_STATE. */
int sdr_graph_batches(sdr_bank *bank);
int sdr_graph_capture(sdr_bank *bank, int n_frames);
/* iq_dev: sdr_graph_batches() device pointers, one batch each, layout and alignment as sdr_process_device. */
int sdr_graph_launch(sdr_bank *bank, const float *const *iq_dev);
/* The same for sc16 input (sdr_process_device_sc16's layout).  A graph runs the format it was captured for: launching it
 * with the other call returns SDR_ERR_STATE. */
int sdr_graph_capture_sc16(sdr_bank *bank, int n_frames);
int sdr_graph_launch_sc16(sdr_bank *bank, const int16_t *const *iq_dev);
/* The same for 8-bit input (sdr_process_device_iq8's layout and formats).  The graph remembers its format: a launch with
 * another one (cs8 against cu8 included) returns SDR_ERR_STATE and names the right call. */
int sdr_graph_capture_iq8(sdr_bank *bank, int n_frames, int format);
int sdr_graph_launch_iq8(sdr_bank *bank, const void *const *iq_dev, int format);
/* Back to sdr_process_*: drains the pipeline, moves what was not polled yet to the host-side queue (sdr_poll keeps
 * delivering it, oldest first) and frees the replays' buffer sets; what the last replay's last batch left on the device
 * goes with them - read it (sdr_read_*) before the release. */
int sdr_graph_release(sdr_bank *bank);

/* several GPUs, one process ------------------------------------------------------------------ */
/* An sdr_group drives one sdr_bank per member - a member is a HIP device ordinal; the same ordinal may repeat (two banks
 * on one device) - as ONE bank of cfg->n_bands bands: band b lives on member b % n_members as local band b / n_members
 * (sharding.bands_of_rank).  Every member gets the rest of *cfg unchanged (geometry, listeners, capacities, find_peaks,
 * trace); cfg->device_id is ignored; n_bands < n_members is SDR_ERR_BAD_ARG.  Semantics are the bank's unless stated:
 *   - per-band calls (sdr_attach, sdr_attach_at, sdr_detach, sdr_listener_stop, sdr_set_center_frequency, sdr_read_*,
 *     sdr_scope_*) go to the member bank and local band sdr_group_member names;
 *   - sdr_group_process_staged(_limit) takes the minimum of staged frames over ALL the group's bands and every member
 *     processes that many, so frame indices, cumulation boundaries and batch_index agree across the group;
 *   - sdr_group_process_device takes one device pointer per member, each laid out as sdr_process_device's over the
 *     member's local bands; every member is enqueued before the call waits for anything;
 *   - the setters apply to every member before the next process call: every band changes at the same frame
 *     (band = -1: every band); timing and refusals are the bank's (sdr_set_*), and sdr_group_set_signal_debounce with a
 *     batch waiting for its listen half returns SDR_ERR_STATE before any member changes;
 *   - sdr_group_poll delivers batch k once every member has finished it, merged into one sdr_results with global band
 *     numbers in exactly one bank's order (chunks by band, then chunk; listeners by band, then slot), first_peak /
 *     first_edge / first_rune renumbered, drop counters summed.  A member batch already taken from its bank is kept by
 *     the group through SDR_ERR_WOULD_BLOCK (another member is behind) and SDR_ERR_BAD_SIZE (n_* set, nothing
 *     delivered); the next call delivers the same batch whole.  Members that disagree on batch_index, first_frame or
 *     n_frames: SDR_ERR_STATE.  sdr_group_poll_peaks is the chunks / peaks half of the same merge.
 * Threading is the bank's: one producer thread, plus one consumer thread in sdr_group_poll.  Every group call leaves the
 * caller's current HIP device as it found it.  The processing calls check every member (listen half pending, graph
 * captured, pointers) before any member is launched; a failure after that (SDR_ERR_HIP) marks the group failed and its
 * processing calls return SDR_ERR_STATE from then on rather than run the members out of step.  Graph mode is not
 * offered: a member captured through sdr_group_member makes the processing calls return SDR_ERR_STATE.  Nor are
 * overlapped frames yet: sdr_group_create with 0 < cfg->hop < block_size returns SDR_ERR_BAD_ARG. */
typedef struct sdr_group sdr_group;
int sdr_group_create(const sdr_config *cfg, const int32_t *device_ids, int n_members, sdr_group **out);
int sdr_group_destroy(sdr_group *group);
int sdr_group_member(sdr_group *group, int band, sdr_bank **bank, int *local_band);
int sdr_group_push_iq(sdr_group *group, int band, int sample_rate, const float *iq, size_t n_floats);
int sdr_group_push_kiwi_snd(sdr_group *group, int band, int sample_rate, const uint8_t *payload, size_t n_bytes);
int sdr_group_process_staged(sdr_group *group, int *n_frames_out);
int sdr_group_process_staged_limit(sdr_group *group, int max_frames, int *n_frames_out);
int sdr_group_process_device(sdr_group *group, const float *const *iq_dev, int n_frames);
/* sc16 input (sdr_push_iq_sc16 / sdr_process_device_sc16), routed exactly like the float32 calls. */
int sdr_group_push_iq_sc16(sdr_group *group, int band, int sample_rate, const int16_t *iq, size_t n_values);
int sdr_group_process_device_sc16(sdr_group *group, const int16_t *const *iq_dev, int n_frames);
/* 8-bit input (sdr_push_iq8 / sdr_process_device_iq8), routed exactly like the float32 calls. */
int sdr_group_push_iq8(sdr_group *group, int band, int sample_rate, const void *iq, size_t n_values, int format);
int sdr_group_process_device_iq8(sdr_group *group, const void *const *iq_dev, int n_frames, int format);
int sdr_group_sync(sdr_group *group);
int sdr_group_set_peak_threshold(sdr_group *group, int band, float threshold);
int sdr_group_set_signal_debounce(sdr_group *group, int band, int debounce);
int sdr_group_set_edge_width(sdr_group *group, int edge_width);
int sdr_group_set_find_peaks(sdr_group *group, int on);
/* sdr_set_first_frame on every member (arguments and statuses are its).  Members given different first frames by hand,
 * through sdr_group_member, disagree on first_frame: sdr_group_poll returns SDR_ERR_STATE. */
int sdr_group_set_first_frame(sdr_group *group, int64_t frame);
/* sdr_set_window on every member, before the group's next process call: every band changes at the same frame, and the
 * members cannot come to disagree (what one would refuse is refused before any member's table changes). */
int sdr_group_set_window(sdr_group *group, const float *window, int n);
int sdr_group_enable_results(sdr_group *group, int on);
int sdr_group_poll(sdr_group *group, sdr_results *results, int wait);
/* sdr_enable_rows on every member, before the group's next process call (what a member would refuse is refused before any
 * member changes; SDR_ERR_STATE also while a group batch is half delivered).  sdr_group_poll_rows: the rows of the oldest
 * batch EVERY member has finished, merged into the order sdr_group_poll gives that batch's chunks (global band, then
 * chunk); the following sdr_group_poll delivers the same batch.  Statuses as sdr_poll_rows / sdr_group_poll. */
int sdr_group_enable_rows(sdr_group *group, int columns);
int sdr_group_poll_rows(sdr_group *group, float *rows, int rows_cap, int *n_rows, int64_t *batch_index, int wait);
/* sdr_enable_reports on every member (refusals as sdr_group_enable_rows).  sdr_group_poll_reports: the reports of the oldest
 * batch EVERY member has finished, merged into one bank's order (global band, then listener id) with global band numbers;
 * the following sdr_group_poll delivers the same batch.  Statuses as sdr_poll_reports / sdr_group_poll. */
int sdr_group_enable_reports(sdr_group *group, int on);
int sdr_group_poll_reports(sdr_group *group, sdr_listener_report *out, int cap, int *n_out, int64_t *batch_index, int wait);
int sdr_group_defer_listen(sdr_group *group, int on);
int sdr_group_poll_peaks(sdr_group *group, sdr_results *results, int wait);
int sdr_group_process_listen(sdr_group *group);
int sdr_group_read_drop_counters(sdr_group *group, uint64_t *runes_dropped, uint64_t *edges_dropped);

/* down-converter ----------------------------------------------------------------------------- */
/* A digital down-converter (DDC) in front of a bank: one WIDE stream - a HackRF's 8-20 MS/s, an RTL-SDR's 2.4 MS/s - goes in
 * once, in any of the four complex input formats or as real samples (below), and n_bands narrow float32 streams come out in device memory, laid out as
 * sdr_process_device_stream reads them.  Each band is mixed to 0 Hz, low-pass filtered and decimated by one kernel.  An
 * sdr_ddc is an object of its own beside the bank; a process that never creates one runs exactly what it ran.  Like the
 * window and the hop it has no counterpart in the reference: its arithmetic is defined here to the bit (DESIGN.md section
 * 1; tests/ddc_ref.py restates it in NumPy), and everything behind it is the reference fed with these float32 samples.
 *
 * The wide stream is x[k], k a 64-bit sample index counted from the DDC's start (or from sdr_ddc_set_first_sample);
 * x[k] = 0 for k below the first sample.  A sample's float32 value (re, im) is what the bank's calls make of that format:
 * exact for cs8 / cu8, float32(x) / 32767 correctly rounded for sc16.  L = SDR_DDC_NCO_SIZE = 65536.  Per band b:
 *   NCO     step_b in [-32768, 32767] tunes the band: a signal step_b * input_rate / L Hz from the wide stream's centre
 *           lands on 0 Hz.  p = (k * step_b) mod L from the full 64-bit k (two's complement for negative steps; the phase
 *           is never truncated: no phase-truncation spurs), c = COS[p], s = SIN[p] from the float32 table of
 *           sdr_ddc_nco_table.
 *   mix     yre = (re * c) + (im * s),  yim = (im * c) - (re * s)  in float32, every operation rounded on its own.
 *   filter  the n_taps float32 taps h are the caller's (as the window is) and the same for every band; with decimation D,
 *           output n is  acc = +0.0f; for j = 0 .. n_taps - 1, in this order: acc = acc + (h[j] * y[n * D - j])
 *           for re and im separately, each product and each sum rounded once in float32; subnormals are kept.
 *   count   a call that brings m * D new samples produces exactly m outputs per band, n = K / D .. K / D + m - 1 for K
 *           samples seen before it.  The DDC keeps the last n_taps - 1 RAW samples on the device between calls and mixes
 *           them again from their absolute index: any cut of a stream into calls gives the same bits, and a retune
 *           between two calls is well defined - an output uses, for all its taps, the step current in the call that
 *           produces it.
 * Calls and statuses (a refused call changes nothing):
 *   sdr_ddc_create       taps: n_taps float32 values, nco_steps: n_bands steps, both copied.  SDR_ERR_BAD_ARG: a null
 *                        pointer, a wrong struct_size, n_bands outside 1..64, decimation outside 1..256, n_taps outside
 *                        1..4096, an unknown in_format, max_in_samples < decimation or not a multiple of it, a non-zero
 *                        reserved word, a step outside [-32768, 32767].
 *   sdr_ddc_set_stream   run on this hipStream_t (NULL = the null stream): the stream the bank's FFT runs on
 *                        (sdr_set_stream), so that a DDC call and the bank call behind it need no synchronisation.
 *   sdr_ddc_set_first_sample  the next sample gets index k0 (k0 >= 0 and a multiple of the decimation, SDR_ERR_BAD_ARG
 *                        otherwise); before the first process call only, SDR_ERR_STATE afterwards.  Mirrors
 *                        sdr_set_first_frame.
 *   sdr_ddc_total_samples  the index of the next sample.
 *   sdr_ddc_set_nco_step from the next process call on.  SDR_ERR_BAD_ARG: band or step out of range.
 *   sdr_ddc_process_device  asynchronous on the DDC's stream.  in_dev: n_in_samples samples of in_format in device memory;
 *                        out_dev: float32 I,Q in device memory, band b's m outputs from sample b * band_stride_samples on.
 *                        Both 16-byte aligned, band_stride_samples a multiple of 4 and >= m (SDR_ERR_BAD_ARG otherwise).
 *                        n_in_samples is a positive multiple of the decimation, at most max_in_samples (SDR_ERR_BAD_SIZE
 *                        otherwise).  Placement in a ring and continuity are the caller's business, as for
 *                        sdr_process_device_stream: the next call's out_dev is where this call's outputs ended.
 *   sdr_ddc_process_host the same with the wide stream in host memory (borrowed for the call), uploaded raw: one byte per
 *                        value for the 8-bit formats.
 *   sdr_ddc_nco_table    host only, needs no handle and no GPU: COS and SIN, SDR_DDC_NCO_SIZE float32 values each (either
 *                        pointer may be null).  Built in float64 from one quarter wave and extended by exact symmetry:
 *                        SIN[i] == COS[(i - L/4) mod L], COS[i] == COS[L - i], COS[i] == -COS[L/2 - i]; exactly 0 and
 *                        +-1 at the multiples of L/4.
 *
 * Real input (SDR_DDC_REAL), for direct-sampling receivers whose ADC delivers one value per sample: a real stream v[k] is
 * the complex stream x[k] = (v[k], +0.0f) through the arithmetic above, bit for bit - the same NCO, the same two mix
 * formulas with im = +0.0f, the same filter order, zeros below the first sample, the same carry of n_taps - 1 RAW samples;
 * signs of zero, NaN and Inf follow from that.  The value of a raw word is what the complex format of the same sample
 * type gives that word: float32 as it is (RF32), float32(x) / 32767 (RS16), x / 128 (RS8), (2 x - 255) / 256 (RU8).
 * Calls, statuses and alignment are unchanged; n_in_samples counts samples, so a call of n samples reads 4 n, 2 n or n
 * bytes, and sdr_ddc_process_host uploads exactly those.
 *   tuning  for a real stream sampled at fs, a signal at f Hz, 0 < f < fs / 2, lands on 0 Hz with
 *           step = round(f * L / fs), which lies in [0, 32767].  A carrier A cos(..) comes out as a complex carrier of
 *           amplitude A / 2 (-6.02 dB); the bank's thresholds are relative to the noise floor and need no change.
 *   mirror  a negative step selects the mirror image of the same signal: the band's spectrum comes out reversed.  That
 *           is what an inverting Nyquist zone needs; otherwise use positive steps.
 *   image   the other half of the real spectrum lies 2 f away after the mix: the caller's taps must reject it, as the
 *           filter's shape is the caller's business throughout.
 * Not offered: per-band taps, resampling by a ratio, DDC launches inside a captured graph, DDCs in an sdr_group, packed
 * 12-bit samples.  (Many equally spaced bands: the channelizer below.) */
#define SDR_DDC_F32 0
#define SDR_DDC_SC16 1
#define SDR_DDC_CS8 2
#define SDR_DDC_CU8 3
#define SDR_DDC_REAL 16 /* flag: one value per sample, no imaginary part */
#define SDR_DDC_RF32 16 /* SDR_DDC_REAL | SDR_DDC_F32 : float32                          */
#define SDR_DDC_RS16 17 /* SDR_DDC_REAL | SDR_DDC_SC16: int16, value float32(x) / 32767  */
#define SDR_DDC_RS8 18  /* SDR_DDC_REAL | SDR_DDC_CS8 : int8,  value x / 128             */
#define SDR_DDC_RU8 19  /* SDR_DDC_REAL | SDR_DDC_CU8 : uint8, value (2 x - 255) / 256   */
#define SDR_DDC_NCO_SIZE 65536
/* outputs of one band that one workgroup of the kernel computes (csrc/ddc.h): where the tests put their output counts */
#define SDR_DDC_TILE_OUTPUTS 512

typedef struct sdr_ddc sdr_ddc;

typedef struct sdr_ddc_config {
    int32_t struct_size;    /* = sizeof(sdr_ddc_config), ABI guard                    */
    int32_t n_bands;        /* 1 .. 64                                                */
    int32_t decimation;     /* D, 1 .. 256                                            */
    int32_t n_taps;         /* T, 1 .. 4096                                           */
    int32_t in_format;      /* SDR_DDC_F32 / _SC16 / _CS8 / _CU8, _RF32 .. _RU8 real  */
    int32_t max_in_samples; /* capacity: input samples per call, a multiple of D      */
    int32_t device_id;      /* HIP device ordinal                                     */
    int32_t reserved;       /* 0                                                      */
} sdr_ddc_config;

int sdr_ddc_create(const sdr_ddc_config *cfg, const float *taps, const int32_t *nco_steps, sdr_ddc **out);
int sdr_ddc_destroy(sdr_ddc *ddc);
int sdr_ddc_sync(sdr_ddc *ddc);
int sdr_ddc_set_stream(sdr_ddc *ddc, void *hip_stream);
int sdr_ddc_set_first_sample(sdr_ddc *ddc, int64_t k0);
int64_t sdr_ddc_total_samples(sdr_ddc *ddc);
int sdr_ddc_set_nco_step(sdr_ddc *ddc, int band, int step);
int sdr_ddc_process_device(sdr_ddc *ddc, const void *in_dev, size_t n_in_samples, float *out_dev, size_t band_stride_samples);
int sdr_ddc_process_host(sdr_ddc *ddc, const void *in_host, size_t n_in_samples, float *out_dev, size_t band_stride_samples);
int sdr_ddc_nco_table(float *cos_out, float *sin_out);

/* channelizer -------------------------------------------------------------------------------- */
/* A polyphase channelizer: one wide stream into M EQUALLY SPACED bands, fs / M apart, all with the same prototype filter,
 * for T multiply-adds and one M-point FFT per output time where the DDC spends n_bands * T.  It is an object of its own
 * beside the DDC and the bank and mirrors sdr_ddc_* call for call; a process that never creates one runs exactly what it
 * ran.  Like the DDC it has no counterpart in the reference: its arithmetic is defined here to the bit (tests/chan_ref.py
 * restates it in NumPy), and everything behind it is the reference fed with these float32 streams.
 *
 * L = SDR_DDC_NCO_SIZE, COS and SIN the tables of sdr_ddc_nco_table.  M = n_channels, D = decimation, T = n_taps = P * M,
 * h[0 .. T-1] the caller's float32 taps.  x[k] is the float32 complex value of stream sample k, exactly what the DDC makes
 * of each SDR_DDC_* input format (a real format is (v, +0.0f)), and (+0, +0) below the first sample; k is a 64-bit index
 * and output time n is absolute, n = k / D.  Per output time n, three steps in this order:
 *   branch sums  for r = 0 .. M-1, for re and im separately: acc = +0.0f; for p = 0 .. P-1, in this order:
 *                acc = acc + (h[r + p * M] * x[n * D - r - p * M]); u[r] = acc.  Every product and every sum is rounded
 *                once in float32; subnormals are kept.
 *   rotation     v[r] = u[(r + n * D) mod M], n * D from the full 64-bit index: the exact replacement of the phase factor
 *                e^{-j 2 pi c n D / M}, without arithmetic.
 *   FFT          M points, kernel e^{+j 2 pi c r / M}, radix 2, decimation in time, unnormalised: a[i] = v[bitrev(i)]; for
 *                len = 2, 4, .. M, every block start s (a multiple of len) and q = 0 .. len/2 - 1:
 *                    w = (COS[q * L / len], SIN[q * L / len]),  lo = a[s + q],  hi = a[s + q + len/2]
 *                    t.re = (w.re * hi.re) - (w.im * hi.im),  t.im = (w.re * hi.im) + (w.im * hi.re)
 *                    a[s + q] = lo + t,  a[s + q + len/2] = lo - t
 *                every operation rounded on its own and no product skipped: the twiddles (1, 0) and (0, 1) are multiplied
 *                like any other (skipping them changes zero signs and what Inf and NaN do).  Channel c's output is a[c].
 * In exact arithmetic channel c is the DDC's band with step = c * L / M (steps above 32767 wrap by -L: channel M/2 is step
 * -32768), the same D and taps: channel c is centred c * fs / M above the wide stream's centre for c < M/2 and
 * (c - M) * fs / M for c >= M/2.  The prototype filter must cut off at half the OUTPUT rate fs / D, as with the DDC.
 * Limits (SDR_ERR_BAD_ARG otherwise): M a power of two in 2 .. 256; D one of M, M/2, M/4 (critically sampled, 2x and 4x
 * oversampled) and at least 1; T = P * M with 1 <= P <= 64 and T <= 4096; n_out in 1 .. M; the channels distinct and in
 * 0 .. M-1 (NULL: channels 0 .. n_out-1).
 * Output stream i is channel channels[i], from float32 I,Q sample i * band_stride_samples of out_dev on: the layout
 * sdr_process_device_stream reads.  Only the listed channels are written: a caller with real input asks for channels
 * 0 .. M/2 only, and nobody pays the HBM writes of channels he does not read.
 * Everything else is the DDC's: the alignment and stride rules, n_in_samples a positive multiple of D and at most
 * max_in_samples (SDR_ERR_BAD_SIZE), sdr_chan_set_first_sample (k0 >= 0, a multiple of D, before the first process call
 * only), a refused call changes nothing, the carry of T - 1 RAW samples on the device, and any cut of the stream into calls
 * gives the same bits.
 *   sdr_chan_tile_outputs  host only, needs no handle and no GPU: the output times one workgroup of the kernel computes for
 *                        this geometry (where the tests put their output counts); negative for a geometry outside the limits.
 * Not offered: per-channel taps, M not a power of two, a channelizer inside a captured graph or an sdr_group, feeding
 * sdr_push_*, library-designed prototype filters, retuning (a channelizer has no NCO: fine tuning between channel centres
 * is the fine converter's job, sdr_fine_* below, which reads the channelizer's outputs where they lie). */
typedef struct sdr_chan sdr_chan;

typedef struct sdr_chan_config {
    int32_t struct_size;    /* = sizeof(sdr_chan_config), ABI guard                   */
    int32_t n_channels;     /* M, a power of two, 2 .. 256                            */
    int32_t decimation;     /* D: M, M/2 or M/4, at least 1                           */
    int32_t n_taps;         /* T = P * M, 1 <= P <= 64, T <= 4096                     */
    int32_t in_format;      /* SDR_DDC_F32 / _SC16 / _CS8 / _CU8, _RF32 .. _RU8 real  */
    int32_t max_in_samples; /* capacity: input samples per call, a multiple of D      */
    int32_t device_id;      /* HIP device ordinal                                     */
    int32_t n_out;          /* output streams written, 1 .. M                         */
} sdr_chan_config;

int sdr_chan_create(const sdr_chan_config *cfg, const float *taps, const int32_t *channels, sdr_chan **out);
int sdr_chan_destroy(sdr_chan *chan);
int sdr_chan_sync(sdr_chan *chan);
int sdr_chan_set_stream(sdr_chan *chan, void *hip_stream);
int sdr_chan_set_first_sample(sdr_chan *chan, int64_t k0);
int64_t sdr_chan_total_samples(sdr_chan *chan);
int sdr_chan_process_device(sdr_chan *chan, const void *in_dev, size_t n_in_samples, float *out_dev, size_t band_stride_samples);
int sdr_chan_process_host(sdr_chan *chan, const void *in_host, size_t n_in_samples, float *out_dev, size_t band_stride_samples);
int sdr_chan_tile_outputs(int n_channels, int decimation, int n_taps);

/* IQ correction ------------------------------------------------------------------------------ */
/* A zero-IF receiver's wide stream has a DC offset (an unkeyed carrier on the stream's centre) and an I/Q gain and phase
 * imbalance (a mirror image of every station at minus its offset, about 30 dB down for 5 % and 3 degrees).  Both are taken
 * out where the DDC's and the channelizer's kernels convert a raw sample, and the values are computed from exact sums of
 * the raw stream.  Everything here is additive: an object that never calls these launches exactly the kernels it launched.
 * The entry points share the prefix sdr_iq_ and take the handle of either object (sdr_iq_ddc_*, sdr_iq_chan_*): the sets of
 * sdr_ddc_* and sdr_chan_* calls stay the ten and nine they were.
 *
 * The correction.  Let (re0, im0) be what the input format makes of a raw word (above).  Each line is one float32
 * operation, rounded on its own:
 *     re1 = re0 - dc_re          im1 = im0 - dc_im
 *     re  = re1                  im  = (gain_im * im1) + (cross * re1)
 * A corrected stream is the stream of these (re, im) through the arithmetic of the DDC or the channelizer as stated above,
 * bit for bit (tests/ddc_ref.py and tests/chan_ref.py fed the corrected float32 values; tests/iqc_ref.py restates the four
 * lines).  Samples below the first sample stay (+0, +0): they are not -dc.
 *   sdr_iq_ddc_set_correction, sdr_iq_chan_set_correction   the four values are copied by the call and hold from the next
 *                        process call on, for every sample that call converts - the n_taps - 1 carried RAW samples
 *                        included, which are read again with the new values.  With constant values any cut of the stream
 *                        into calls gives the same bits.  A change between two calls is well defined: an output uses, for all
 *                        its taps, the values current in the call that produces it (as for sdr_ddc_set_nco_step), so the
 *                        n_taps - 1 samples around a change are seen once with the old and once with the new values.
 *                        NULL: no correction, the kernels and the bits of an object that never set one.  The identity
 *                        (0, 0, 1, 0) is NOT "none": it runs the corrected kernels, and its bits differ for a sample that is
 *                        -0 (-0 - 0 is -0 but 0 * re1 may turn a sum's zero sign) or not finite (0 * Inf is NaN).
 *                        SDR_ERR_BAD_ARG: a null handle, a field that is not finite, an object with a real input format
 *                        (SDR_DDC_REAL).  A refused call changes nothing.
 *
 * The sums.  For SDR_DDC_CS8, _CU8 and _SC16 (SDR_ERR_BAD_ARG for _F32 - such a caller has floats in hand - and for the real
 * formats) an object can sum the raw stream in integer units u: cs8 x, cu8 2 x - 255, sc16 x.
 *   sdr_iq_*_enable_sums on != 0: from the next process call on, every accepted call also sums its own n_in_samples raw
 *                        samples, each sample of the stream once; the carry is never summed and a correction is ignored.
 *                        Off in a new object; switching off, and switching on, clear the sums.
 *   sdr_iq_*_read_sums   waits for the object's stream, returns the sums since the last read (or since they were switched
 *                        on) and clears them.  SDR_ERR_STATE while the sums are off.
 * All six values are exact integers: any kernel schedule and any cut of the stream into calls give the same bits.  A call
 * that would take n past 2^32 since the last read is not summed; its samples are counted in `skipped` (so sum_ii and sum_qq
 * stay within 2^62).
 *   sdr_iq_correction_from_sums   host only, needs no handle and no GPU.  Defined operation by operation in float64, each
 *                        rounded once (NumPy reproduces its bits); S = 128 (cs8), 256 (cu8), 32767 (sc16):
 *                            N = (double)n;  mi = (double)sum_i / N;  mq = (double)sum_q / N
 *                            vi = (double)sum_ii / N - mi * mi;  vq = (double)sum_qq / N - mq * mq
 *                            c = (double)sum_iq / N - mi * mq
 *                            r = vq - (c * c) / vi;  g = sqrt(vi / r);  x = -(g * (c / vi))
 *                            dc_re = (float)(mi / S);  dc_im = (float)(mq / S);  gain_im = (float)g;  cross = (float)x
 *                        SDR_ERR_BAD_ARG, with *out untouched: a null pointer, n < 2, vi <= 0, r <= 0, an intermediate that
 *                        is not finite, any other in_format.
 * What the estimate assumes: a stream whose TRUE I and Q are uncorrelated and of equal power.  Noise and any sum of
 * stations at different offsets satisfy that; a single strong carrier exactly on the centre does not.  The estimate is
 * blind and per call of read: smooth the values on the host before setting them.
 * Not offered: corrections per band or per frequency, a tracking loop on the device, sums of float32 or real streams, DC
 * removal for real formats, a correction for the bank's own *_iq8 / *_sc16 calls. */
typedef struct sdr_iq_correction {
    float dc_re, dc_im, gain_im, cross;
} sdr_iq_correction; /* 16 bytes */

typedef struct sdr_iq_sums { /* 64 bytes; raw integer units u: cs8 x, cu8 2 x - 255, sc16 x */
    int64_t n, sum_i, sum_q, sum_ii, sum_qq, sum_iq;
    int64_t skipped;  /* samples of calls that were not summed (n would have passed 2^32) */
    int64_t reserved; /* 0 */
} sdr_iq_sums;

int sdr_iq_ddc_set_correction(sdr_ddc *ddc, const sdr_iq_correction *c);
int sdr_iq_ddc_enable_sums(sdr_ddc *ddc, int on);
int sdr_iq_ddc_read_sums(sdr_ddc *ddc, sdr_iq_sums *out);
int sdr_iq_chan_set_correction(sdr_chan *chan, const sdr_iq_correction *c);
int sdr_iq_chan_enable_sums(sdr_chan *chan, int on);
int sdr_iq_chan_read_sums(sdr_chan *chan, sdr_iq_sums *out);
int sdr_iq_correction_from_sums(const sdr_iq_sums *s, int in_format, sdr_iq_correction *out);

/* impulse noise blanker ---------------------------------------------------------------------- */
/* Impulse noise (power lines, ignition, electric fences, switching supplies) is a burst of a few samples at the wide rate,
 * tens of dB above the band; behind the DDC's or the channelizer's filter it is that filter's impulse response in every
 * band.  The blanker removes it before any narrow filter has seen it: raw samples in, raw samples of the SAME format out,
 * both in device memory.  Its output goes to sdr_ddc_process_device, sdr_chan_process_device or, for a receiver that feeds
 * the bank directly, sdr_process_device_stream_sc16 / _iq8.  An sdr_nb is an object of its own (a sample's fate depends on
 * its neighbourhood, so it is no per-word input trait as the IQ correction is); a process that never creates one launches
 * exactly what it launched.  It has no counterpart in the reference: its arithmetic is defined here in integers, to the bit
 * (tests/nb_ref.py restates it), and everything behind it is the existing path fed with the blanked samples.
 *
 *   formats   SDR_DDC_SC16, _CS8, _CU8, _RS16, _RS8, _RU8.
 *   unit      a raw value's integer unit u is the one of sdr_iq_sums: x for int8 and int16, 2 x - 255 for uint8.  A sample's
 *             squared magnitude is m[k] = uI^2 + uQ^2 (complex), u^2 (real).
 *   index     k is a 64-bit sample index counted from the object's start (or from sdr_nb_set_first_sample).
 *   config    block B: a power of two, 64 .. 4096; window W: a power of two, 1 .. 64; B * W <= 65536.
 *   power     block j holds samples j B .. j B + B - 1;  P[j] = sum of m[k] over the block, an exact integer (<= 2^43).
 *   level     R[j] = P[j-W] + .. + P[j-1].  Only blocks with W full blocks of this stream behind them are judged: samples of
 *             the first W blocks after the start are never impulses.
 *   impulse   sample k of a judged block j is an impulse iff   m[k] * (B * W) * 16 > ratio_q4 * R[j]   in unsigned 64-bit
 *             integers.  ratio_q4 is the power ratio over the window's mean, in sixteenths, 16 .. 16384; the left side stays
 *             below 2^52 and the right side below 2^62 (static assertions in csrc/host/nb_rule.h).  ratio_q4 = 0 switches
 *             judging off: nothing is an impulse, powers are still tracked.  R[j] = 0 needs no rule: the inequality decides.
 *   gate      sample k is blanked iff some impulse i has i <= k <= i + hold, 0 <= hold <= B.  The gate crosses block ends
 *             and call ends.  An impulse is judged with the R of its own block and with the ratio_q4 current in the call
 *             that brought it; a gate that runs into the next call keeps the length it had.
 *   blank     a blanked sample is written as: 0 in both parts for int8 and int16; I = 127 + (k & 1), Q = 128 - (k & 1) for
 *             cu8; 127 + (k & 1) for ru8 (u = -+1, +-1: zero on average, since uint8 has no zero).  Every other sample is
 *             copied byte for byte.
 *   calls     n_in_samples is a positive multiple of B, at most max_in_samples.  The object keeps the last W block powers
 *             and the open gate's remaining length on the device between calls; no call waits for the device.  Any cut of
 *             a stream into calls gives the same output bytes and the same statistics.
 *   stats     `impulses` (samples judged impulses) and `blanked` (samples replaced) are exact 64-bit totals counted on the
 *             device, `samples` the host's count of samples seen; sdr_nb_read_stats waits for the stream, returns all three
 *             since the last read and clears them.  The blanked share is how a user sets ratio_q4.
 * Calls and statuses (a refused call changes nothing):
 *   sdr_nb_create        SDR_ERR_BAD_ARG: a null pointer, a wrong struct_size, a format, block, window, ratio_q4 or hold
 *                        outside the above, max_in_samples < B or not a multiple of it.
 *   sdr_nb_set_stream    the stream of the DDC and the bank, so that no synchronisation is needed between them.
 *   sdr_nb_set_first_sample  k0 >= 0 and a multiple of B (SDR_ERR_BAD_ARG), before the first process call only
 *                        (SDR_ERR_STATE).  The warm-up of W blocks starts at k0.
 *   sdr_nb_set_threshold ratio_q4 and hold from the next process call on.  SDR_ERR_BAD_ARG outside the ranges.
 *   sdr_nb_process_device  asynchronous on the blanker's stream.  in_dev and out_dev: n_in_samples samples of in_format, both
 *                        16-byte aligned, and the two ranges must not overlap (SDR_ERR_BAD_ARG: the gate reads samples in
 *                        front of the ones it writes, so operation in place is undefined).  SDR_ERR_BAD_SIZE: a length that
 *                        is not a positive multiple of B, or above max_in_samples.
 *   sdr_nb_process_host  the same with the input in host memory (borrowed for the call), uploaded raw through pinned memory.
 *   sdr_nb_tile_samples  host only, needs no handle and no GPU: the samples one workgroup of the gate kernel writes (where
 *                        the tests put their lengths); negative for a format or block outside the above.
 *   sdr_nb_blank_host    host only, needs no GPU: the definition over one whole stream from k = 0, in plain C++ with
 *                        integers; cfg as for sdr_nb_create (device_id is ignored, n_in_samples may exceed max_in_samples),
 *                        in and out in host memory and not overlapping, stats may be null.
 * Not offered: float32 streams (SDR_DDC_F32, _RF32: SDR_ERR_BAD_ARG), a reference level that excludes blanked samples,
 * median or minimum references, per-band blanking behind the DDC, interpolation across the gap instead of the blank word, a
 * gate that opens before the impulse (it would cost latency), lengths that are not multiples of B, blanker launches inside a
 * captured graph or in an sdr_group, an automatic threshold. */
typedef struct sdr_nb sdr_nb;

typedef struct sdr_nb_config {
    int32_t struct_size;    /* = sizeof(sdr_nb_config), ABI guard                     */
    int32_t in_format;      /* SDR_DDC_SC16 / _CS8 / _CU8 / _RS16 / _RS8 / _RU8       */
    int32_t block;          /* B, a power of two, 64 .. 4096                          */
    int32_t window;         /* W, a power of two, 1 .. 64, B * W <= 65536             */
    int32_t ratio_q4;       /* 16 .. 16384 (sixteenths of the window's mean), 0: off  */
    int32_t hold;           /* 0 .. B: samples blanked behind an impulse              */
    int32_t max_in_samples; /* capacity: input samples per call, a multiple of B      */
    int32_t device_id;      /* HIP device ordinal                                     */
} sdr_nb_config; /* 32 bytes */

typedef struct sdr_nb_stats {
    int64_t samples, impulses, blanked, reserved;
} sdr_nb_stats; /* 32 bytes */

int sdr_nb_create(const sdr_nb_config *cfg, sdr_nb **out);
int sdr_nb_destroy(sdr_nb *nb);
int sdr_nb_sync(sdr_nb *nb);
int sdr_nb_set_stream(sdr_nb *nb, void *hip_stream);
int sdr_nb_set_first_sample(sdr_nb *nb, int64_t k0);
int64_t sdr_nb_total_samples(sdr_nb *nb);
int sdr_nb_set_threshold(sdr_nb *nb, int ratio_q4, int hold);
int sdr_nb_process_device(sdr_nb *nb, const void *in_dev, size_t n_in_samples, void *out_dev);
int sdr_nb_process_host(sdr_nb *nb, const void *in_host, size_t n_in_samples, void *out_dev);
int sdr_nb_read_stats(sdr_nb *nb, sdr_nb_stats *out);
int sdr_nb_tile_samples(int in_format, int block);
int sdr_nb_blank_host(const sdr_nb_config *cfg, const void *in, size_t n_in_samples, void *out, sdr_nb_stats *stats);

/* fine converter ----------------------------------------------------------------------------- */
/* A second stage behind the channelizer or a first DDC: n_bands output bands in one launch, each band reading its OWN
 * stage-one output stream, tuned with the DDC's NCO and decimated again.  Chained behind a channelizer it puts bands anywhere
 * in the wide stream at the channelizer's cost; behind a DDC it reaches total decimations up to 65536; a station that drifts
 * across a channel edge is followed by re-pointing its band.  An sdr_fine is an object of its own beside the DDC, the
 * channelizer and the bank; a process that never creates one launches exactly what it launched (no existing launcher is
 * touched).  Its arithmetic is the down-converter's, bit for bit (tests/fine_ref.py restates it over tests/ddc_ref.py).
 *
 *   input    n_inputs streams of float32 I,Q in device memory, stream i from sample i * in_stride_samples of in_dev on: the
 *            layout sdr_chan_process_device and sdr_ddc_process_device write, so stage one's band_stride_samples is stage
 *            two's in_stride_samples and nothing is copied.  All inputs share one 64-bit sample index k, counted from the
 *            object's start (or from sdr_fine_set_first_sample); every stream is zero below the first sample.
 *   band     band b is the down-converter's arithmetic above applied to stream inputs[b] with step nco_steps[b]: the same
 *            table and phase p = (k * step) mod L from the full k, the same two mix formulas, acc = +0.0f and
 *            acc = acc + (h[j] * y[n * D - j]) for j = 0 .. n_taps - 1 with every product and sum rounded once, subnormals
 *            kept.  It is exactly what a one-band SDR_DDC_F32 sdr_ddc gives when fed that stream.  A step tunes by
 *            step * (input rate) / 65536 Hz.  Several bands may read one input; an input may go unread.
 *   state    the device keeps the last n_taps - 1 raw samples of EVERY input between calls (double-buffered, as the DDC's
 *            carry is), whether a band reads that input or not: any cut of the streams into calls gives the same bits, and a
 *            band moved to another input finds that input's history.  sdr_fine_set_nco_step and sdr_fine_set_input hold
 *            from the next process call on; an output uses, for all its taps, the step and the input current in the call that
 *            produces it.
 * Calls and statuses (these mirror sdr_ddc_*; a refused call changes nothing):
 *   sdr_fine_create      taps: n_taps float32 values; nco_steps: n_bands steps; inputs: n_bands input indices, or NULL for
 *                        band b reads input b (which needs n_bands <= n_inputs); all copied.  SDR_ERR_BAD_ARG: a null
 *                        config, taps, steps or output, a wrong struct_size, n_bands outside 1..64, n_inputs outside 1..256,
 *                        decimation outside 1..256, n_taps outside 1..4096, max_in_samples < decimation or not a multiple of
 *                        it, a non-zero reserved word, a step outside [-32768, 32767], an input outside 0 .. n_inputs - 1.
 *   sdr_fine_set_stream  the stream stage one and the bank run on, so that the three calls need no synchronisation.
 *   sdr_fine_set_first_sample  k0 >= 0 and a multiple of the decimation (SDR_ERR_BAD_ARG), before the first process call
 *                        only (SDR_ERR_STATE).  Behind a stage one that started at K0 with decimation D1 it is K0 / D1.
 *   sdr_fine_total_samples  the index of the next sample (of every input).
 *   sdr_fine_set_nco_step, sdr_fine_set_input   SDR_ERR_BAD_ARG: band, step or input out of range.
 *   sdr_fine_process_device  asynchronous on the object's stream.  n_in_samples new samples of every input; band b's
 *                        m = n_in_samples / decimation outputs go to float32 I,Q sample b * band_stride_samples of out_dev
 *                        on.  in_dev and out_dev 16-byte aligned, in_stride_samples a multiple of 4 and >= n_in_samples,
 *                        band_stride_samples a multiple of 4 and >= m (SDR_ERR_BAD_ARG otherwise); n_in_samples a positive
 *                        multiple of the decimation, at most max_in_samples (SDR_ERR_BAD_SIZE otherwise).  out_dev must not
 *                        overlap in_dev: the kernel reads the inputs while it writes the outputs, and this cannot be checked.
 *   sdr_fine_tune        host only, needs no handle and no GPU, exact in integers: where to point a band behind a channelizer
 *                        of M = n_channels channels with decimation D.  target is the wanted band centre in units of
 *                        wide_rate / (65536 * D), the fine step's own unit.  With q = 65536 * D / M (an integer), c is
 *                        target / q rounded to nearest, ties toward the even channel, and step = target - c * q; a step of
 *                        32768 (possible only at D = M) becomes channel c + 1 and step -32768.  *channel = c mod M in
 *                        0 .. M - 1, *step = the step.  SDR_ERR_BAD_ARG with the outputs untouched: a null output, M not a
 *                        power of two in 2 .. 256 or D not one of M, M/2, M/4 and at least 1 (the channelizer's limits),
 *                        |target| > 32768 * D (outside the wide stream).  In exact arithmetic channel c followed by this
 *                        step equals one DDC of the wide stream whose total mix is target / (65536 * D) cycles per sample.
 * Not offered: input formats other than float32, a host entry point (the input is device-resident by construction), per-band
 * taps or decimations, IQ correction and sums on this object, launches inside a captured graph, sdr_group. */
typedef struct sdr_fine sdr_fine;

typedef struct sdr_fine_config {
    int32_t struct_size;    /* = sizeof(sdr_fine_config), ABI guard                   */
    int32_t n_bands;        /* 1 .. 64 output bands                                   */
    int32_t n_inputs;       /* 1 .. 256 input streams (a channelizer's n_out, a DDC's n_bands) */
    int32_t decimation;     /* D, 1 .. 256                                            */
    int32_t n_taps;         /* T, 1 .. 4096, one filter for every band                */
    int32_t max_in_samples; /* per input stream and call, a multiple of D             */
    int32_t device_id;      /* HIP device ordinal                                     */
    int32_t reserved;       /* 0                                                      */
} sdr_fine_config; /* 32 bytes */

int sdr_fine_create(const sdr_fine_config *cfg, const float *taps, const int32_t *nco_steps, const int32_t *inputs, sdr_fine **out);
int sdr_fine_destroy(sdr_fine *f);
int sdr_fine_sync(sdr_fine *f);
int sdr_fine_set_stream(sdr_fine *f, void *hip_stream);
int sdr_fine_set_first_sample(sdr_fine *f, int64_t k0);
int64_t sdr_fine_total_samples(sdr_fine *f);
int sdr_fine_set_nco_step(sdr_fine *f, int band, int step);
int sdr_fine_set_input(sdr_fine *f, int band, int input);
int sdr_fine_process_device(sdr_fine *f, const float *in_dev, size_t in_stride_samples, size_t n_in_samples,
                            float *out_dev, size_t band_stride_samples);
int sdr_fine_tune(int n_channels, int decimation, int64_t target, int32_t *channel, int32_t *step);

/* receive chain ------------------------------------------------------------------------------ */
/* One call from raw samples to bank batches.  An sdr_chain joins objects the caller created and still owns,
 *     [sdr_nb] -> sdr_ddc | sdr_chan -> [sdr_fine] -> sdr_bank        (the parts in brackets are optional)
 * and does what INTEGRATION.md's hand-written loops leave to the integrator: pushes of ANY length, a bounded ring in device
 * memory, the carry between calls, the pointers' alignment and the frame arithmetic.  It launches no DSP kernel of its own:
 * the hot path is the five launchers above (sdr_nb_process_device, sdr_ddc_ / sdr_chan_process_device,
 * sdr_fine_process_device, sdr_process_device_stream), and the chain only decides pointers and counts and moves a carry.  A
 * process that never creates a chain calls exactly what it called.  Every narrow sample and every result is what the
 * hand-written sequence gives for the same stream, bit for bit, whatever the push lengths are.
 *
 * The plan (csrc/host/chain_plan.h; tests/chain_ref.py restates it).  D1 is stage one's decimation, Dtot = D1 times the fine
 * converter's decimation (Dtot = D1 without one).  WIDE samples are the raw stream's, NARROW samples one band's at the bank.
 *   granule   G = lcm(2 * Dtot, the blanker's block (1 without a blanker), 16).  The factor 2 makes every piece produce an
 *             even number of narrow samples, which keeps every stage's float32 I,Q output pointer 16-byte aligned; the 16
 *             keeps a piece's first sample 16-byte aligned for one-byte real formats.  sdr_chain_granule returns it.
 *   piece     the largest multiple of G that fits every member's max_in_samples (the blanker's, stage one's, and the fine
 *             converter's counted times D1).
 *   ring      linear, per band: band b's samples start at b * ring_samples; it holds narrow samples [base, have) of the
 *             chain's stream (indices count from the chain's creation).  ring_samples >= 2 * block_size + piece / Dtot
 *             rounded up to a multiple of 4 (sdr_chain_min_ring; 0 in the configuration selects that minimum).
 *   push_host takes ANY n_samples in 1 .. max_in_samples, borrowed for the call only.  The samples go through the chain's
 *             pinned memory into its raw device buffer, behind the `pending` samples (always fewer than G) a former push
 *             left.  The largest multiple of G now there is processed in pieces of at most `piece`; the rest stays pending
 *             and is moved to the buffer's front by a device copy (which cannot overlap: what was processed is at least G,
 *             what moves is less).
 *   push_device  reads the caller's device memory in place: n_samples a positive multiple of G, at most max_in_samples
 *             (SDR_ERR_BAD_SIZE), raw_dev 16-byte aligned (SDR_ERR_BAD_ARG), and nothing pending (SDR_ERR_STATE).  The
 *             memory must stay untouched until the work enqueued has run (sdr_chain_sync, or the stream's own order).
 *   a piece   of p wide samples: the blanker writes it into a chain-owned buffer; stage one writes its p / D1 outputs per
 *             stream to the front of a chain-owned buffer, or straight into the ring when there is no fine converter; the
 *             fine converter writes into the ring.  m = p / Dtot new narrow samples per band land behind the ones there.
 *   carry     before a piece, if have - base + m > ring_samples, the unconsumed samples [next, have), next = frames * hop
 *             with `frames` the frames processed so far - fewer than block_size of them - are moved to the ring's front
 *             by one strided device-to-device copy on the stream, and base = next.
 *   batches   after each piece, while have - next >= block_size: one sdr_process_device_stream of
 *             min((have - next - block_size) / hop + 1, max_batch_frames) frames at ring offset next - base.
 *             *n_batches (may be null) is the number of bank batches the push enqueued: what sdr_poll will deliver.
 * Which batches a push enqueues is thereby a function of the geometry and the push lengths alone.  Everything is
 * asynchronous on ONE stream; a push returns without a device synchronisation, except that push_host waits until its own
 * pinned buffer is free, as sdr_ddc_process_host does.
 *
 * Members stay usable.  sdr_fine_set_nco_step / sdr_fine_set_input, sdr_ddc_set_nco_step, sdr_iq_*, sdr_nb_set_threshold /
 * sdr_nb_read_stats, every setter of the bank, sdr_attach / sdr_detach and sdr_poll* are called on the member handles
 * between pushes and hold "from the next process call on": from the first wide sample not yet processed, pending samples
 * included (sdr_chain_stats says how many are pending).  Driving a member's PROCESS call directly while it is in a chain is
 * an error the chain notices: it remembers every member's *_total_samples / sdr_total_frames behind its own calls, and a
 * push that finds one changed returns SDR_ERR_STATE and does nothing.
 * Calls and statuses (a refused call changes nothing):
 *   sdr_chain_create     SDR_ERR_BAD_ARG: a null pointer, a wrong struct_size, a non-zero reserved word, max_in_samples < 1, no
 *                        bank, both or neither of ddc and chan, a blanker whose in_format is not stage one's, a fine
 *                        converter whose n_inputs is not stage one's output count (a DDC's n_bands, a channelizer's n_out),
 *                        a last stage whose band count is not the bank's n_bands, members on different devices or on
 *                        different streams (the chain runs on the stream its members share), piece < G, a ring_samples
 *                        that is neither 0 nor a multiple of 4 of at least sdr_chain_min_ring.  SDR_ERR_STATE: a bank with
 *                        a graph captured, with input staged (sdr_push_*), or with sdr_defer_listen on.
 *   sdr_chain_destroy    waits for the stream and frees the chain's buffers; the members stay the caller's, in the state
 *                        the chain left them, and can be driven by hand from then on.
 *   sdr_chain_set_stream the chain's stream and, through their own set_stream calls, every member's.
 *   sdr_chain_sync       every member's sync.
 *   sdr_chain_push_host, sdr_chain_push_device   SDR_ERR_BAD_SIZE: n_samples 0 or above max_in_samples (and the rule
 *                        above); SDR_ERR_STATE: a member was driven directly, or a member's call failed half way through
 *                        an earlier push (destroy the chain).
 *   sdr_chain_read_narrow  for recording and for tests: waits for the stream and copies narrow samples [from, from + n) of
 *                        `band` to out_host (2 n floats).  SDR_ERR_BAD_ARG unless base <= from, n >= 1 and
 *                        from + n <= have: only resident samples can be read.
 *   sdr_chain_stats      counters kept on the host; it does not wait for the device.
 *   sdr_chain_granule, sdr_chain_min_ring   host only, need no handle and no GPU; negative for an argument below 1, a hop
 *                        above block_size or a piece that is no multiple of total_decimation.
 * Not offered: chains in a captured graph or an sdr_group; a bank fed in raw sc16 or iq8 without a stage one; deferred
 * listening; a call that inserts zeros for samples the receiver dropped; an IQ-correction or blanker-threshold loop run by
 * the chain; several chains into one bank; set_first_sample through the chain (set it on the members before creating the
 * chain). */
typedef struct sdr_chain sdr_chain;

typedef struct sdr_chain_config {
    int32_t struct_size;     /* = sizeof(sdr_chain_config), ABI guard                    */
    int32_t max_in_samples;  /* per push, wide samples                                   */
    int32_t ring_samples;    /* narrow samples per band held in HBM; 0 = the minimum     */
    int32_t reserved;        /* 0                                                        */
    sdr_nb *nb;              /* or NULL                                                  */
    sdr_ddc *ddc;            /* exactly one of ddc / chan                                */
    sdr_chan *chan;
    sdr_fine *fine;          /* or NULL                                                  */
    sdr_bank *bank;
} sdr_chain_config; /* 56 bytes with 8-byte pointers */

typedef struct sdr_chain_counts { /* 96 bytes */
    int64_t accepted;     /* wide samples taken by pushes                             */
    int64_t processed;    /* ... of which went through the stages                     */
    int64_t pending;      /* ... of which wait in the raw buffer: accepted - processed */
    int64_t narrow;       /* narrow samples produced per band (`have`)                */
    int64_t frames;       /* frames the bank was given                                */
    int64_t batches;      /* bank batches enqueued                                    */
    int64_t carry_moves;  /* times the ring's unconsumed samples moved to its front   */
    int64_t granule;      /* G                                                        */
    int64_t piece;        /* wide samples per piece at the most                       */
    int64_t ring_samples; /* the ring size in use                                     */
    int64_t resident_from; /* `base`: the first narrow sample sdr_chain_read_narrow can still read */
    int64_t reserved;     /* 0                                                        */
} sdr_chain_counts;

int sdr_chain_create(const sdr_chain_config *cfg, sdr_chain **out);
int sdr_chain_destroy(sdr_chain *chain);
int sdr_chain_set_stream(sdr_chain *chain, void *hip_stream);
int sdr_chain_sync(sdr_chain *chain);
int sdr_chain_push_host(sdr_chain *chain, const void *raw, size_t n_samples, int *n_batches);
int sdr_chain_push_device(sdr_chain *chain, const void *raw_dev, size_t n_samples, int *n_batches);
int sdr_chain_read_narrow(sdr_chain *chain, int band, int64_t from, int n, float *out_host);
int sdr_chain_stats(sdr_chain *chain, sdr_chain_counts *out);
int64_t sdr_chain_granule(int total_decimation, int nb_block);
int64_t sdr_chain_min_ring(int block_size, int hop, int64_t piece, int total_decimation);

/* scope tap ---------------------------------------------------------------------------------- */
/* The reference shows its inner workings through scope.Scope (scope/scope.go:33-37); NullScope is the default
 * and so is "no tap" here: the two reads below need a bank created with trace = 1 (that is scope.Active()).
 * A frame's Timestamp is replaced by the frame index, everything else is the reference's payload:
 *   stream "spectrum" (rx/receiver.go:428-457): once per completed cumulation, Values = cumulation / 100 as
 *       float64, FrequencyMarkers{"signal_bin"} = bin of the first listener (-1: none),
 *       MagnitudeMarkers{"threshold"} = peakThreshold, FromFrequency 0, ToFrequency 1;
 *   stream "demod" (cw/spectral.go:56-81): once per listener per frame, Values{"threshold", "value",
 *       "state" (-1 / 100), "debounced" (-1 / 80)}. */
typedef struct sdr_scope_spectral_frame {
    int64_t frame;          /* bank frame index that completed the cumulation */
    double from_frequency;  /* 0 */
    double to_frequency;    /* 1 */
    double signal_bin;      /* FrequencyMarkers["signal_bin"] */
    double threshold;       /* MagnitudeMarkers["threshold"] */
    int32_t n_values;       /* block_size */
    int32_t reserved;
} sdr_scope_spectral_frame;

typedef struct sdr_scope_time_frame {
    double threshold, value, state, debounced;
} sdr_scope_time_frame;

/* 1 if the bank taps (created with trace = 1), else 0: scope.Scope.Active(). */
int sdr_scope_active(sdr_bank *bank);
/* Spectral frame of completed cumulation `chunk` of the last batch; values: float64[block_size]. */
int sdr_scope_read_spectral(sdr_bank *bank, int band, int chunk, sdr_scope_spectral_frame *frame, double *values, int max_values);
/* The listener's "demod" time frames of the last batch, one per frame. */
int sdr_scope_read_demod(sdr_bank *bank, int band, int listener_id, sdr_scope_time_frame *out, int max, int *n_out);
/* cw.Decoder's scope streams (cw/decode.go:228-243, :433-491) for the last batch, one record per tick the listener
 * took: scopeDecode {duration, on_threshold, state}, scopeSignalTiming {on_duration = state ? duration : 0, on_threshold,
 * _low, _high, 2 x _high, state}, scopeGapTiming {off_duration = state ? 0 : duration, off_threshold, _low, _high,
 * 2 x _high - threshold, state}, scopeSignal {state}: every channel is one of these fields or a sum of two.  *n_out: the
 * number of ticks (a listener bound inside the batch has fewer than the batch has frames).  trace == 1 only. */
typedef struct sdr_scope_decode_frame {
    int64_t frame;     /* bank frame index of the tick */
    double duration;   /* currentDuration: ticks since the last edge */
    double state;      /* 0 / 1 */
    double on_threshold, on_threshold_low, on_threshold_high;
    double off_threshold, off_threshold_low, off_threshold_high;
} sdr_scope_decode_frame;
int sdr_scope_read_decode(sdr_bank *bank, int band, int listener_id, sdr_scope_decode_frame *out, int max, int *n_out);

/* measurement ------------------------------------------------------------------------------- */
/* When enabled every kernel launch is bracketed by HIP events on the bank's stream. */
int sdr_profile_enable(sdr_bank *bank, int on);
/* kernel: 0 fft_project, 1 window_means, 2 noise_stats, 3 thresholds, 4 listen_gather,
 *         5 cumulate, 6 find_peaks, 7 listen_decode, 8 cum_rows (sdr_enable_rows; no launch while rows are off),
 *         9 listen_report, 10 report_marks (sdr_enable_reports; no launch while reports are off).
 * Returns accumulated milliseconds and launch count. */
int sdr_profile_read(sdr_bank *bank, int kernel, double *total_ms, int *launches);
int sdr_profile_reset(sdr_bank *bank);
const char *sdr_kernel_name(int kernel);

/* audio path (cw/audio.go): n_streams mono float32 streams, one Goertzel + debouncer + decoder each */
typedef struct sdr_audio sdr_audio;
int sdr_audio_create(int n_streams, double pitch, int sample_rate, int max_blocks, int device_id, sdr_audio **out);
int sdr_audio_destroy(sdr_audio *a);
int sdr_audio_blocksize(sdr_audio *a);
int sdr_audio_set_scale(sdr_audio *a, double scale);             /* 0 = autoscale (audio.go:184-187) */
int sdr_audio_set_debounce(sdr_audio *a, int threshold);          /* default 3 (audio.go:18)          */
int sdr_audio_set_magnitude_threshold(sdr_audio *a, double t);    /* default 0.75 (dsp.go:12)         */
/* Feed n_samples mono float32 samples per stream (host memory, layout [stream][n_samples]); whole
 * Goertzel blocks are processed, the remainder is kept for the next call (audio.go:175-179). */
int sdr_audio_write(sdr_audio *a, const float *samples, int n_samples);
int sdr_audio_close(sdr_audio *a);                                /* decoder.stop (audio.go:205-207)  */
/* The text one stream decoded since the last read, as UTF-8; a rune is never split (the decoder emits two-byte
 * runes, U+00A7 and U+00A6, for keying it cannot name).  What does not fit into max_bytes is kept, in order, for the
 * next call.  A stream stores at most 4096 undelivered runes: those decoded while the store is full are dropped. */
int sdr_audio_read_text(sdr_audio *a, int stream, char *out, int max_bytes, int *n_bytes);
/* per-block normalised magnitude / raw / debounced state of the last write (parity) */
int sdr_audio_read_trace(sdr_audio *a, int stream, double *magnitudes, uint8_t *raw, uint8_t *debounced, int max,
                         int *n_blocks);

#ifdef __cplusplus
}
#endif
#endif /* SDRAINER_HIP_H */
