// syldet_stream.cpp -- the streaming front end: the producers' appends, the pump, and what the consumer reads.

#include "syldet_handle.hpp"

// one callback buffer of a channel: Double(sum) / Double(length) into its input statistic (Processor.swift:111-113)
template <class T>
static void meter_input(syldet *h, int channel, const T *data, int64_t n, int64_t step)
{
    const double v = (double)sum_squares_tree(data, n, step) / (double)n;
    syldet::Meter &m = *h->meters[(size_t)channel];
    std::lock_guard<std::mutex> lock(m.mu);
    syldet::Meter::write(m.in_has, m.in_cur, v);
}

// (T: float, or int16_t converted on the way into the fp32 ring: x * 2^-15, exact; the ring's room is counted as for fp32)
template <class T>
static int append_impl(syldet *h, int32_t channel, const T *data, int64_t n_samples)
{
    if (!h || channel < 0 || channel >= h->channels || n_samples < 0 || (n_samples > 0 && !data))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    ChannelStream &cs = *h->streams[(size_t)channel];
    if (!cs.has_room(n_samples, h->geom.hop)) return fail(SYLDET_ERR_BUFFER_FULL, "Insufficient space on buffer.");
    if (!cs.ensure_ring()) return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    if (n_samples > 0 && h->meters_on.load(std::memory_order_acquire)) meter_input(h, channel, data, n_samples, 1);
    cs.write(data, n_samples, 1);
    return SYLDET_OK;
}

// source: channel c takes slot source[c] of every frame (syldet_append_interleaved_channels); null: slot c of frames that hold
// exactly the bank's channels
template <class T>
static int append_interleaved_impl(syldet *h, const T *data, int64_t n_frames, int32_t total_channels, const int32_t *source = nullptr)
{
    if (!h || n_frames < 0 || (n_frames > 0 && !data) || (source ? total_channels < 1 : total_channels != h->channels))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    for (int c = 0; source && c < h->channels; c++)
        if (source[c] < 0 || source[c] >= total_channels) return fail(SYLDET_ERR_INVALID_ARGUMENT, "source channel outside the stream");
    // all channels or none: a caller that retries after "buffer full" must not double a block on some of them
    // (room only grows between the check and the writes: the consumer is the only other party)
    for (int c = 0; c < h->channels; c++)
        if (!h->streams[(size_t)c]->has_room(n_frames, h->geom.hop)) return fail(SYLDET_ERR_BUFFER_FULL, "Insufficient space on buffer.");
    for (int c = 0; c < h->channels; c++)
        if (!h->streams[(size_t)c]->ensure_ring()) return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    if (n_frames > 0 && h->meters_on.load(std::memory_order_acquire))
        for (int c = 0; c < h->channels; c++) meter_input(h, c, data + (source ? source[c] : c), n_frames, total_channels);
    for (int c = 0; c < h->channels; c++) h->streams[(size_t)c]->write(data + (source ? source[c] : c), n_frames, total_channels);
    return SYLDET_OK;
}

// Evaluates what the listed channels have pending: channels with the same number of new evaluations share one
// pinned staging block, one H2D copy, one launch and one D2H copy; the results join each channel's queue of
// computed evaluations.  Adds the number queued to *queued.
static int pump_impl(syldet *h, const int32_t *channels, int32_t n, int64_t *queued)
{
    std::lock_guard<std::mutex> pump_lock(h->pump_mu);
    const int n_out = h->geom.outputs;
    const int64_t hop = h->geom.hop, frame = (int64_t)h->geom.gap + h->cfg.view.window_length;
    std::map<int64_t, std::vector<int32_t>> groups;          // evaluations -> channels
    for (int32_t i = 0; i < n; i++) {
        ChannelStream &cs = *h->streams[(size_t)channels[i]];
        const uint64_t tail = cs.tail.load(std::memory_order_acquire);
        // `while processFourierData() {}` (SyllableDetector.swift:155): every whole frame is extracted now
        cs.frames_done.store(count_frames(h, (int64_t)tail), std::memory_order_release);
        const int64_t E = count_evals(h, (int64_t)(tail - cs.head.load(std::memory_order_relaxed)));
        if (E > 0) groups[E].push_back(channels[i]);
    }
    if (groups.empty()) return SYLDET_OK;
    SYLDET_HIP(hipSetDevice(h->device));
    const bool mixed = !h->classes.empty();
    for (auto &g : groups) {
        const int64_t E = g.first, S = frame + (E + h->cfg.view.time_range - 2) * hop;   // samples E evaluations span
        const size_t nc = g.second.size();
        // a mixed bank: the group's rows ordered by class, so that each class's launch reads and writes a contiguous slice; the
        // class-local networks of the rows travel behind the samples in the same copy
        const size_t tab = mixed ? nc * sizeof(int) : 0;
        if (mixed) std::stable_sort(g.second.begin(), g.second.end(), [h](int32_t a, int32_t b) { return h->class_of[(size_t)a] < h->class_of[(size_t)b]; });
        if (int st = h->p_stage_in.reserve(nc * (size_t)S * sizeof(float) + tab)) return st;
        if (int st = h->p_stage_out.reserve(nc * (size_t)E * (size_t)n_out * sizeof(float))) return st;
        if (int st = h->d_stage_in.reserve(nc * (size_t)S * sizeof(float) + tab)) return st;
        if (int st = h->d_stage_out.reserve(nc * (size_t)E * (size_t)n_out * sizeof(float))) return st;
        float *in = (float *)h->p_stage_in.ptr, *outs = (float *)h->p_stage_out.ptr;
        for (size_t k = 0; k < nc; k++) {
            const ChannelStream &cs = *h->streams[(size_t)g.second[k]];
            cs.copy_out(cs.head.load(std::memory_order_relaxed), in + k * (size_t)S, (size_t)S);
        }
        if (mixed) {
            int *nets = reinterpret_cast<int *>(in + nc * (size_t)S);
            for (size_t k = 0; k < nc; k++) {
                const syldet &cl = *h->classes[(size_t)h->class_of[(size_t)g.second[k]]];
                nets[k] = cl.n_nets > 1 ? cl.net_of[(size_t)h->local_of[(size_t)g.second[k]]] : 0;
            }
            SYLDET_HIP(hipMemcpyAsync(h->d_stage_in.ptr, in, nc * (size_t)S * sizeof(float) + tab, hipMemcpyHostToDevice, h->stream));
            h->prof_begin();                                         // (one call: every class's launches)
            const int *d_nets = reinterpret_cast<const int *>((const float *)h->d_stage_in.ptr + nc * (size_t)S);
            for (size_t k0 = 0; k0 < nc;) {
                const int cls = h->class_of[(size_t)g.second[k0]];
                size_t k1 = k0;
                while (k1 < nc && h->class_of[(size_t)g.second[k1]] == cls) k1++;
                syldet *cl = h->classes[(size_t)cls].get();
                if (int st = run_on_stream(cl, (const float *)h->d_stage_in.ptr + k0 * (size_t)S, S, S, (int)(k1 - k0),
                                           (float *)h->d_stage_out.ptr + k0 * (size_t)E * (size_t)n_out, nullptr, h->stream,
                                           cl->n_nets > 1 ? d_nets + k0 : nullptr))
                    return st;
                k0 = k1;
            }
        } else {
            SYLDET_HIP(hipMemcpyAsync(h->d_stage_in.ptr, in, nc * (size_t)S * sizeof(float), hipMemcpyHostToDevice, h->stream));
            // (a multi-network handle: the networks of the channels this launch carries, in its row order; the vector outlives the
            // copy -- the stream is synchronised below)
            std::vector<int> rows_net;
            if (h->n_nets > 1) {
                for (size_t k = 0; k < nc; k++) rows_net.push_back(h->net_of[(size_t)g.second[k]]);
                if (int st = h->d_stage_net.reserve(nc * sizeof(int))) return st;
                SYLDET_HIP(hipMemcpyAsync(h->d_stage_net.ptr, rows_net.data(), nc * sizeof(int), hipMemcpyHostToDevice, h->stream));
            }
            if (int st = run_on_stream(h, (const float *)h->d_stage_in.ptr, S, S, (int)nc, (float *)h->d_stage_out.ptr, nullptr, h->stream,
                                       h->n_nets > 1 ? (const int *)h->d_stage_net.ptr : nullptr))
                return st;
        }
        SYLDET_HIP(hipMemcpyAsync(outs, h->d_stage_out.ptr, nc * (size_t)E * (size_t)n_out * sizeof(float), hipMemcpyDeviceToHost,
                                  h->stream));
        SYLDET_HIP(hipStreamSynchronize(h->stream));
        for (size_t k = 0; k < nc; k++) {
            ChannelStream &cs = *h->streams[(size_t)g.second[k]];
            const float *o = outs + k * (size_t)E * (size_t)n_out;
            {
                std::lock_guard<std::mutex> lock(cs.mu);
                for (int64_t e = 0; e < E; e++) cs.ready.emplace_back(o + (size_t)e * (size_t)n_out, o + (size_t)(e + 1) * (size_t)n_out);
            }
            // each evaluation consumes one column = hop samples (:175-178)
            cs.head.store(cs.head.load(std::memory_order_relaxed) + (uint64_t)(E * hop), std::memory_order_release);
            if (queued) *queued += E;
        }
    }
    return SYLDET_OK;
}

static int pump(syldet *h, const int32_t *channels, int32_t n, int64_t *queued)
{
    try {                                                        // no exception crosses the C boundary
        return pump_impl(h, channels, n, queued);
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
}

extern "C" {

// ---- streaming front-end -------------------------------------------------------------
// The reference keeps, per detector, a 409600-byte sample ring drained one frame at a
// time and a feature ring of F-float columns drained one column per evaluation.  Here a
// channel keeps the raw samples from the first frame of its next evaluation onward; when
// the consumer asks for a value and none is queued, every evaluation those samples allow
// is computed in one device pass and queued.  Results are the batch engine's.

int syldet_append(syldet_t *h, int32_t channel, const float *data, int64_t n_samples)
{
    return append_impl(h, channel, data, n_samples);
}

int syldet_append_s16(syldet_t *h, int32_t channel, const int16_t *data, int64_t n_samples)
{
    return append_impl(h, channel, data, n_samples);
}

int syldet_append_interleaved(syldet_t *h, const float *data, int64_t n_frames, int32_t total_channels)
{
    return append_interleaved_impl(h, data, n_frames, total_channels);
}

int syldet_append_interleaved_s16(syldet_t *h, const int16_t *data, int64_t n_frames, int32_t total_channels)
{
    return append_interleaved_impl(h, data, n_frames, total_channels);
}

int syldet_append_interleaved_channels(syldet_t *h, const float *data, int64_t n_frames, int32_t total_channels, const int32_t *source_channel)
{
    if (!source_channel) return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    return append_interleaved_impl(h, data, n_frames, total_channels, source_channel);      // (all channels or none, as syldet_append_interleaved)
}

int syldet_process_new_value(syldet_t *h, int32_t channel)
{
    if (!h || channel < 0 || channel >= h->channels) return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    ChannelStream &cs = *h->streams[(size_t)channel];
    if (int st = pump(h, &channel, 1, nullptr)) return st;
    float out0;
    {
        std::lock_guard<std::mutex> lock(cs.mu);
        if (cs.ready.empty()) return 0;
        cs.last = std::move(cs.ready.front());
        cs.ready.pop_front();
        out0 = cs.last[0];
    }
    if (h->meters_on.load(std::memory_order_acquire)) {              // Processor.swift:138
        syldet::Meter &m = *h->meters[(size_t)channel];
        std::lock_guard<std::mutex> lock(m.mu);
        syldet::Meter::write(m.out_has, m.out_cur, (double)out0);
    }
    return 1;
}

int syldet_process_all(syldet_t *h, int64_t *n_queued)
{
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    std::vector<int32_t> all;
    try {
        all.resize((size_t)h->channels);
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    for (int32_t c = 0; c < h->channels; c++) all[(size_t)c] = c;
    int64_t queued = 0;
    if (int st = pump(h, all.data(), h->channels, &queued)) return st;
    if (n_queued) *n_queued = queued;
    return SYLDET_OK;
}

int64_t syldet_pending_evaluations(const syldet_t *h, int32_t channel)
{
    if (!h || channel < 0 || channel >= h->channels) return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    ChannelStream &cs = *h->streams[(size_t)channel];
    std::lock_guard<std::mutex> lock(cs.mu);
    return (int64_t)cs.ready.size();
}

int syldet_last_outputs(const syldet_t *h, int32_t channel, float *out)
{
    if (!h || !out || channel < 0 || channel >= h->channels) return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    ChannelStream &cs = *h->streams[(size_t)channel];
    std::lock_guard<std::mutex> lock(cs.mu);
    std::copy(cs.last.begin(), cs.last.end(), out);
    return SYLDET_OK;
}

int syldet_last_detected(const syldet_t *h, int32_t channel)
{
    if (!h || channel < 0 || channel >= h->channels) return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    ChannelStream &cs = *h->streams[(size_t)channel];
    std::lock_guard<std::mutex> lock(cs.mu);
    const double thr = h->chan_thr0.empty() ? h->cfg.view.thresholds[0] : h->chan_thr0[(size_t)channel];   // (the channel's own network)
    return (double)cs.last[0] >= thr ? 1 : 0;   // SyllableDetector.swift:27-31
}

int syldet_seen_syllable(syldet_t *h, int32_t channel)
{
    int ret = 0;                                                       // SyllableDetector.swift:220-230
    for (;;) {
        const int r = syldet_process_new_value(h, channel);
        if (r < 0) return r;
        if (r == 0) break;
        if (syldet_last_detected(h, channel) == 1) ret = 1;
    }
    return ret;
}

}  // extern "C"
