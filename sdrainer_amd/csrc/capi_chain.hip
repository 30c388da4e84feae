// capi_chain.hip — the receive chain behind the C ABI (include/sdrainer_hip.h "receive chain"): raw samples in, bank batches
// out.  It borrows a blanker, a stage one (down-converter or channelizer), a fine converter and a bank, and calls their public
// process entry points; it owns a raw buffer (pending samples and host uploads), a clean buffer (the blanker's output), a mid
// buffer (stage one's output in front of a fine converter) and the ring of narrow samples the bank reads.  What a push does is
// host/chain_plan.h's list of actions, executed here in order on the chain's one stream; no kernel is launched in this file.
//
// A push plans on a copy of the state and commits it once every action has been enqueued.  A member that refuses or fails
// half way leaves the members out of step with each other: the chain is marked failed and refuses further pushes.
// The failure function, the HIP-error macro, the guard of a half-built chain and push_host's upload are front.h's, the
// members' own.
#include "chain.h"
#include "front.h"
#include "host/chain_plan.h"

using sdr::fail;

struct sdr_chain {
    sdr_chain_config cfg{};
    sdr::ChainPlan plan;
    hipStream_t stream = nullptr;
    int device = 0;
    int n_bands = 0;         // the bank's, the last stage's
    int n_mid = 0;           // stage one's output streams
    int d1 = 1;              // stage one's decimation
    size_t sample_bytes = 0; // of one raw sample
    size_t mid_stride = 0;   // samples between stage one's output streams in d_mid
    char *d_raw = nullptr;   // [granule + max_in_samples] raw samples: pending ones in front, a host push behind them
    char *d_clean = nullptr; // the blanker's output, one piece
    float *d_mid = nullptr;  // [n_mid][mid_stride] float32 I,Q: stage one's output in front of the fine converter
    float *d_ring = nullptr; // [n_bands][ring] float32 I,Q
    sdr::HostUpload upload;  // push_host's way into d_raw (front.h; allocated by the first such call)
    // the members' counters behind the chain's own calls: a push that finds one changed was overtaken by a direct call
    int64_t seen_nb = 0, seen_one = 0, seen_fine = 0, seen_frames = 0;
    bool failed = false;
};

namespace {

int64_t one_total(const sdr_chain *c) { return c->cfg.ddc ? sdr_ddc_total_samples(c->cfg.ddc) : sdr_chan_total_samples(c->cfg.chan); }

void remember(sdr_chain *c)
{
    c->seen_nb = c->cfg.nb ? sdr_nb_total_samples(c->cfg.nb) : 0;
    c->seen_one = one_total(c);
    c->seen_fine = c->cfg.fine ? sdr_fine_total_samples(c->cfg.fine) : 0;
    c->seen_frames = sdr_total_frames(c->cfg.bank);
}

bool untouched(const sdr_chain *c)
{
    return (!c->cfg.nb || sdr_nb_total_samples(c->cfg.nb) == c->seen_nb) && one_total(c) == c->seen_one &&
           (!c->cfg.fine || sdr_fine_total_samples(c->cfg.fine) == c->seen_fine) && sdr_total_frames(c->cfg.bank) == c->seen_frames;
}

// the actions of one push, in order; `in` is where a piece's offset counts from (the raw buffer, or the caller's memory)
int execute(sdr_chain *c, const std::vector<sdr::ChainAction> &actions, const char *in, int *n_batches)
{
    const sdr_chain_config &m = c->cfg;
    const size_t ring = (size_t)c->plan.g.ring, sb = c->sample_bytes;
    for (const sdr::ChainAction &a : actions) {
        int rc = SDR_OK;
        switch (a.op) {
        case sdr::ChainOp::Upload:
            break;  // (enqueued by sdr_chain_push_host, in front of everything)
        case sdr::ChainOp::Piece: {
            const void *src = in + (size_t)a.a * sb;
            const size_t p = (size_t)a.b;
            float *ring_at = c->d_ring + 2 * (size_t)a.c;
            if (m.nb) {
                if ((rc = sdr_nb_process_device(m.nb, src, p, c->d_clean)))
                    return rc;
                src = c->d_clean;
            }
            float *out1 = m.fine ? c->d_mid : ring_at;
            const size_t stride1 = m.fine ? c->mid_stride : ring;
            rc = m.ddc ? sdr_ddc_process_device(m.ddc, src, p, out1, stride1) : sdr_chan_process_device(m.chan, src, p, out1, stride1);
            if (rc)
                return rc;
            if (m.fine && (rc = sdr_fine_process_device(m.fine, c->d_mid, c->mid_stride, p / (size_t)c->d1, ring_at, ring)))
                return rc;
            break;
        }
        case sdr::ChainOp::Move:
            HIP_TRY(hipSetDevice(c->device));
            if (a.c > 0)
                HIP_TRY(hipMemcpy2DAsync(c->d_ring + 2 * (size_t)a.b, ring * sizeof(float2), c->d_ring + 2 * (size_t)a.a, ring * sizeof(float2),
                                      (size_t)a.c * sizeof(float2), (size_t)c->n_bands, hipMemcpyDeviceToDevice, c->stream));
            break;
        case sdr::ChainOp::Batch:
            if ((rc = sdr_process_device_stream(m.bank, c->d_ring + 2 * (size_t)a.a, (int)a.b, ring)))
                return rc;
            if (n_batches)
                ++*n_batches;
            break;
        case sdr::ChainOp::Keep:
            HIP_TRY(hipSetDevice(c->device));
            HIP_TRY(hipMemcpyAsync(c->d_raw + (size_t)a.b * sb, c->d_raw + (size_t)a.a * sb, (size_t)a.c * sb, hipMemcpyDeviceToDevice, c->stream));
            break;
        }
    }
    return SDR_OK;
}

int push(sdr_chain *c, const void *raw, size_t n_samples, int *n_batches, bool host)
{
    if (!c || !raw)
        return fail(SDR_ERR_BAD_ARG, "null chain or input");
    if (c->failed)
        return fail(SDR_ERR_STATE, "a member's call failed half way through an earlier push; destroy the chain");
    const int64_t n = n_samples > (size_t)c->plan.g.max_in ? c->plan.g.max_in + 1 : (int64_t)n_samples;  // (either is refused)
    const sdr::ChainPlan::Refusal why = c->plan.check(n, host);
    if (why == sdr::ChainPlan::BadSize)
        return fail(SDR_ERR_BAD_SIZE, host ? "n_samples must lie in 1 .. max_in_samples"
                                            : "n_samples must be a positive multiple of the granule, at most max_in_samples");
    if (!host && !sdr::aligned16(raw))
        return fail(SDR_ERR_BAD_ARG, "raw_dev must be 16-byte aligned");
    if (why == sdr::ChainPlan::State)
        return fail(SDR_ERR_STATE, "sdr_chain_push_device: samples of a host push are pending (push_host until sdr_chain_stats says 0)");
    if (!untouched(c))
        return fail(SDR_ERR_STATE, "a member's process call was driven directly while it is in the chain");
    sdr::ChainPlan next = c->plan;
    std::vector<sdr::ChainAction> actions;
    next.push(n, host, actions);
    HIP_TRY(hipSetDevice(c->device));
    if (host) {
        const int rc = c->upload.stage(raw, c->sample_bytes * n_samples, c->sample_bytes * (size_t)c->plan.g.max_in,
                                       c->d_raw + (size_t)c->plan.pending * c->sample_bytes, c->stream);
        if (rc)
            return rc;
    }
    if (n_batches)
        *n_batches = 0;
    const int rc = execute(c, actions, host ? c->d_raw : static_cast<const char *>(raw), n_batches);
    if (rc) {
        c->failed = true;  // (sdr_last_error holds the member's message)
        return rc;
    }
    c->plan = next;
    remember(c);
    return SDR_OK;
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

int64_t sdr_chain_granule(int total_decimation, int nb_block) { return sdr::chain_granule(total_decimation, nb_block); }

int64_t sdr_chain_min_ring(int block_size, int hop, int64_t piece, int total_decimation)
{
    return sdr::chain_min_ring(block_size, hop, piece, total_decimation);
}

int sdr_chain_destroy(sdr_chain *c)
{
    if (!c)
        return SDR_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(c->d_raw);
    (void)hipFree(c->d_clean);
    (void)hipFree(c->d_mid);
    (void)hipFree(c->d_ring);
    c->upload.release();
    delete c;
    return SDR_OK;
}

int sdr_chain_create(const sdr_chain_config *cfg, sdr_chain **out)
{
    if (!cfg || !out)
        return fail(SDR_ERR_BAD_ARG, "null config or output");
    if (cfg->struct_size != (int32_t)sizeof(sdr_chain_config))
        return fail(SDR_ERR_BAD_ARG, "sdr_chain_config.struct_size mismatch");
    if (cfg->reserved != 0)
        return fail(SDR_ERR_BAD_ARG, "sdr_chain_config.reserved must be 0");
    if (cfg->max_in_samples < 1)
        return fail(SDR_ERR_BAD_ARG, "max_in_samples must be at least 1");
    if (!cfg->bank)
        return fail(SDR_ERR_BAD_ARG, "a chain ends in a bank");
    if ((cfg->ddc != nullptr) == (cfg->chan != nullptr))
        return fail(SDR_ERR_BAD_ARG, "exactly one of ddc and chan is stage one");
    // stage one, as the chain sees either kind
    int fmt, d1, n_one, dev_one;
    int64_t limit;
    hipStream_t stream;
    if (cfg->ddc) {
        const sdr_ddc_config &o = sdr::ddc_config(cfg->ddc);
        fmt = o.in_format, d1 = o.decimation, n_one = o.n_bands, dev_one = o.device_id, limit = o.max_in_samples;
        stream = sdr::ddc_stream(cfg->ddc);
    } else {
        const sdr_chan_config &o = sdr::chan_config(cfg->chan);
        fmt = o.in_format, d1 = o.decimation, n_one = o.n_out, dev_one = o.device_id, limit = o.max_in_samples;
        stream = sdr::chan_stream(cfg->chan);
    }
    const sdr::ChainBankView bank = sdr::chain_bank_view(cfg->bank);
    bool one_device = dev_one == bank.device_id, one_stream = stream == bank.stream;
    int64_t dtot = d1, nb_block = 1;
    int n_last = n_one;
    if (cfg->nb) {
        const sdr_nb_config &o = sdr::nb_config(cfg->nb);
        if (o.in_format != fmt)
            return fail(SDR_ERR_BAD_ARG, "the blanker's in_format is not stage one's");
        nb_block = o.block;
        limit = o.max_in_samples < limit ? o.max_in_samples : limit;
        one_device = one_device && o.device_id == dev_one;
        one_stream = one_stream && sdr::nb_stream(cfg->nb) == stream;
    }
    if (cfg->fine) {
        const sdr_fine_config &o = sdr::fine_config(cfg->fine);
        if (o.n_inputs != n_one)
            return fail(SDR_ERR_BAD_ARG, "the fine converter's n_inputs is not stage one's output count");
        dtot *= o.decimation;
        n_last = o.n_bands;
        const int64_t wide = (int64_t)o.max_in_samples * d1;
        limit = wide < limit ? wide : limit;
        one_device = one_device && o.device_id == dev_one;
        one_stream = one_stream && sdr::fine_stream(cfg->fine) == stream;
    }
    if (n_last != bank.n_bands)
        return fail(SDR_ERR_BAD_ARG, "the last stage's band count is not the bank's n_bands");
    if (!one_device)
        return fail(SDR_ERR_BAD_ARG, "the members are on different devices");
    if (!one_stream)
        return fail(SDR_ERR_BAD_ARG, "the members are on different streams (set one stream on every member, or sdr_chain_set_stream later)");
    sdr::ChainGeometry g{};
    g.total_decimation = dtot;
    g.granule = sdr::chain_granule(dtot, nb_block);
    g.piece = sdr::chain_piece(g.granule, limit);
    if (g.granule < 1 || g.piece < g.granule)
        return fail(SDR_ERR_BAD_ARG, "not one granule (lcm(2 * total decimation, blanker block, 16)) fits every member's max_in_samples");
    g.block_size = bank.block_size;
    g.hop = bank.hop;
    g.max_batch_frames = bank.max_batch_frames;
    g.max_in = cfg->max_in_samples;
    const int64_t min_ring = sdr::chain_min_ring(g.block_size, g.hop, g.piece, dtot);
    g.ring = cfg->ring_samples == 0 ? min_ring : cfg->ring_samples;
    if (min_ring < 1 || g.ring < min_ring || g.ring % 4 != 0 || g.ring > 0xffffffffll)
        return fail(SDR_ERR_BAD_ARG, "ring_samples must be 0 or a multiple of 4 of at least sdr_chain_min_ring");
    if (bank.graph_captured)
        return fail(SDR_ERR_STATE, "the bank has a graph captured (sdr_graph_release first)");
    if (bank.input_staged)
        return fail(SDR_ERR_STATE, "the bank has input staged (a bank in a chain is fed by the chain alone)");
    if (bank.defer_listen)
        return fail(SDR_ERR_STATE, "the bank defers its listen half (sdr_defer_listen): not offered in a chain");
    HIP_TRY(hipSetDevice(bank.device_id));
    sdr::Building<sdr_chain, sdr_chain_destroy> c(new sdr_chain());
    c->cfg = *cfg;
    c->plan.g = g;
    c->stream = stream;
    c->device = bank.device_id;
    c->n_bands = bank.n_bands;
    c->n_mid = n_one;
    c->d1 = d1;
    c->sample_bytes = (size_t)sdr::ddc_sample_bytes(fmt);
    // the most one piece ever holds: a push processes at most the whole granules of pending + max_in_samples
    const int64_t most = (g.granule - 1 + g.max_in) / g.granule * g.granule, p_cap = most < g.piece ? most : g.piece;
    c->mid_stride = ((size_t)(p_cap / d1) + 3) / 4 * 4;
    HIP_TRY(hipMalloc((void **)&c->d_raw, c->sample_bytes * (size_t)(g.granule + g.max_in)));
    if (cfg->nb)
        HIP_TRY(hipMalloc((void **)&c->d_clean, c->sample_bytes * (size_t)p_cap));
    if (cfg->fine)
        HIP_TRY(hipMalloc((void **)&c->d_mid, sizeof(float2) * c->mid_stride * (size_t)n_one));
    HIP_TRY(hipMalloc((void **)&c->d_ring, sizeof(float2) * (size_t)g.ring * (size_t)bank.n_bands));
    remember(c.get());
    *out = c.release();
    return SDR_OK;
}

int sdr_chain_set_stream(sdr_chain *c, void *hip_stream)
{
    if (!c)
        return fail(SDR_ERR_BAD_ARG, "null chain");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (the ring and the pending samples are ordered by the old stream)
    const sdr_chain_config &m = c->cfg;
    int rc = SDR_OK;
    if (m.nb && (rc = sdr_nb_set_stream(m.nb, hip_stream)))
        return rc;
    if ((rc = m.ddc ? sdr_ddc_set_stream(m.ddc, hip_stream) : sdr_chan_set_stream(m.chan, hip_stream)))
        return rc;
    if (m.fine && (rc = sdr_fine_set_stream(m.fine, hip_stream)))
        return rc;
    if ((rc = sdr_set_stream(m.bank, hip_stream)))
        return rc;
    c->stream = (hipStream_t)hip_stream;
    return SDR_OK;
}

int sdr_chain_sync(sdr_chain *c)
{
    if (!c)
        return fail(SDR_ERR_BAD_ARG, "null chain");
    const sdr_chain_config &m = c->cfg;
    int rc = SDR_OK;
    if (m.nb && (rc = sdr_nb_sync(m.nb)))
        return rc;
    if ((rc = m.ddc ? sdr_ddc_sync(m.ddc) : sdr_chan_sync(m.chan)))
        return rc;
    if (m.fine && (rc = sdr_fine_sync(m.fine)))
        return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return sdr_sync(m.bank);
}

int sdr_chain_push_host(sdr_chain *c, const void *raw, size_t n_samples, int *n_batches) { return push(c, raw, n_samples, n_batches, true); }

int sdr_chain_push_device(sdr_chain *c, const void *raw_dev, size_t n_samples, int *n_batches)
{
    return push(c, raw_dev, n_samples, n_batches, false);
}

int sdr_chain_read_narrow(sdr_chain *c, int band, int64_t from, int n, float *out_host)
{
    if (!c || !out_host)
        return fail(SDR_ERR_BAD_ARG, "null chain or output");
    if (band < 0 || band >= c->n_bands)
        return fail(SDR_ERR_BAD_ARG, "band out of range");
    if (n < 1 || from < c->plan.base || from > c->plan.have - n)
        return fail(SDR_ERR_BAD_ARG, "sdr_chain_read_narrow: the samples are not resident in the ring (sdr_chain_stats: resident_from .. narrow)");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const float *src = c->d_ring + 2 * ((size_t)band * (size_t)c->plan.g.ring + (size_t)(from - c->plan.base));
    HIP_TRY(hipMemcpy(out_host, src, sizeof(float2) * (size_t)n, hipMemcpyDeviceToHost));
    return SDR_OK;
}

int sdr_chain_stats(sdr_chain *c, sdr_chain_counts *out)
{
    if (!c || !out)
        return fail(SDR_ERR_BAD_ARG, "null chain or output");
    const sdr::ChainPlan &p = c->plan;
    *out = sdr_chain_counts{};
    out->accepted = p.accepted;
    out->processed = p.processed;
    out->pending = p.pending;
    out->narrow = p.have;
    out->frames = p.frames;
    out->batches = p.batches;
    out->carry_moves = p.moves;
    out->granule = p.g.granule;
    out->piece = p.g.piece;
    out->ring_samples = p.g.ring;
    out->resident_from = p.base;
    return SDR_OK;
}

#pragma GCC visibility pop
}
