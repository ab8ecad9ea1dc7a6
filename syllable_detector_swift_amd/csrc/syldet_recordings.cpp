// syldet_recordings.cpp -- packed recordings (include/syldet.h, "packed recordings"): the plan that lays many recordings of
// different lengths end to end in a bank's rows, and the handle that keeps the plan's tables on the device so that the
// device calls (kernels_recordings.hip; kernels_recordings_sinc.hip for recordings at other rates; kernels_recordings_pcm.hip for
// the files' own bytes) are launches only.  The handle
// itself is in syldet_recordings.hpp, the layout of its device block in recordings_blob.hpp; its per-sample tracks are in
// syldet_recordings_tracks.cpp, its level meters in syldet_recordings_levels.cpp.
#include <numeric>

#include "recordings_blob.hpp"
#include "syldet_recordings.hpp"

namespace {

using Plan = syldet_recordings::Plan;

static_assert(sizeof(RecSlotDev) == RecBlob::kSlot && sizeof(RecEventDev) == RecBlob::kEvent && sizeof(RecSincDev) == RecBlob::kSinc &&
                  sizeof(RecTrackDev) == RecBlob::kTrack, "recordings_blob.hpp states the tables' entries");

// b: the bank's clock, channels and channel_net (a handle's, or a configuration's: no device either way); p: its host part
int make_plan(const BankInfo &b, const int64_t *n_samples, const int32_t *network, int32_t K, Plan &p)
{
    if (K < 0 || (K > 0 && !n_samples)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "a NULL array or a negative count");
    if (b.channel_net && K > 0 && !network)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "a bank of several networks needs the network of every recording");
    for (int32_t k = 0; k < K; k++) {
        if (n_samples[k] < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_samples[" + std::to_string(k) + "] is negative");
        if (network && network[k] < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "network[" + std::to_string(k) + "] is negative");
        if (!b.channel_net && network && network[k] != 0)
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "network[" + std::to_string(k) + "] on a bank of one network must be 0");
        if (b.channel_net && std::find(b.channel_net, b.channel_net + b.channels, (int)network[k]) == b.channel_net + b.channels)
            return fail(SYLDET_ERR_UNSUPPORTED, "no row of the bank runs network " + std::to_string(network[k]) + " (recording " + std::to_string(k) + ")");
    }
    const int C = b.channels;
    const int64_t hop = b.geom.hop;
    try {
        p.K = K;
        p.slots.assign((size_t)K, syldet_slot_t{});
        std::vector<int64_t> padded((size_t)K), fills((size_t)C, 0);
        std::vector<int32_t> by((size_t)K);
        std::iota(by.begin(), by.end(), 0);
        for (int32_t k = 0; k < K; k++) padded[(size_t)k] = (n_samples[k] + hop - 1) / hop * hop;
        std::stable_sort(by.begin(), by.end(), [&](int32_t a, int32_t c) { return padded[(size_t)a] > padded[(size_t)c]; });
        double total = 0.0;
        for (int32_t k : by) {
            int best = -1;
            for (int c = 0; c < C; c++)
                if ((!b.channel_net || b.channel_net[c] == network[k]) && (best < 0 || fills[(size_t)c] < fills[(size_t)best])) best = c;
            syldet_slot_t &s = p.slots[(size_t)k];
            s.row = best;
            s.offset = fills[(size_t)best];
            s.first_eval = s.offset / hop;
            s.n_evals = count_evals(b.geom, b.window_length, b.time_range, n_samples[k]);
            s.n_samples = n_samples[k];
            fills[(size_t)best] += padded[(size_t)k];
            total += (double)n_samples[k];
        }
        const int64_t most = C > 0 && K > 0 ? *std::max_element(fills.begin(), fills.end()) : 0;
        p.row_samples = (most + 7) / 8 * 8;
        p.row_evals = count_evals(b.geom, b.window_length, b.time_range, p.row_samples);
        p.fill = p.row_samples > 0 ? total / ((double)C * (double)p.row_samples) : 0.0;
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    return SYLDET_OK;
}

int load_impl(syldet_recordings_t *r, const void *d_src, bool s16, const PcmSrc *pcm, const int64_t *src_offset, const int32_t *src_step,
              void *d_rows, int64_t channel_stride, hipStream_t stream)
{
    if (!r || !d_rows || (r->plan.K > 0 && (!d_src || !src_offset || (pcm && !pcm->format)))) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int st = stride_arg(r, channel_stride)) return st;
    if (int st = source_args(r->plan.K, src_offset, src_step)) return st;
    if (pcm)
        if (int st = pcm_args(r->plan.K, d_src, *pcm, src_offset, src_step, [&](int k) { return r->plan.slots[(size_t)k].n_samples; })) return st;
    if (r->plan.row_samples == 0) return SYLDET_OK;
    // the key is the table itself: entry i holds the sources of recording order[i]
    KeptTable<RecSlotDev> &t = r->load.table;
    const std::vector<int32_t> &order = r->plan.order;
    auto step = [&](size_t i) { return step_of(pcm, src_step, order[i]); };
    bool same = t.kept;
    for (size_t i = 0; i < order.size() && same; i++)
        same = t.host[i].src_offset == src_offset[order[i]] && t.host[i].src_step == step(i) && t.host[i].format == format_of(pcm, order[i]);
    SYLDET_HIP(hipSetDevice(r->bank.device));
    if (!same) {
        // new sources: the table is re-made behind the last plain load that reads it
        int st = t.remake([&]() -> int {
            for (size_t i = 0; i < order.size(); i++) {
                t.host[i].src_offset = src_offset[order[i]];
                t.host[i].src_step = step(i);
                t.host[i].format = format_of(pcm, order[i]);
            }
            return SYLDET_OK;
        });
        if (st) return st;
    }
    t.read_on(stream);
    if (!pcm) {
        SYLDET_HIP(launch_recordings_load(r->load.desc, d_src, s16, d_rows, channel_stride, r->bank.channels, stream));
        return SYLDET_OK;
    }
    r->h->prof_begin();
    KernelTimer timer(r->h, stream, "recordings_load_pcm_kernel");
    SYLDET_HIP(launch_recordings_load_pcm(r->load.desc, d_src, (float *)d_rows, channel_stride, r->bank.channels, stream));
    return SYLDET_OK;
}

// ---- the converting load: recordings at other rates brought to the network's as the rows load ----
struct SincLaunch {
    syldet_recordings_t *r;
    const void *d_src;
    bool s16, pcm;
    float *d_rows;
    int64_t stride;
    hipStream_t stream;
};

int sinc_launch(const float *table, int entries, void *ctx)
{
    const SincLaunch &a = *(const SincLaunch *)ctx;
    if (a.pcm)
        SYLDET_HIP(launch_recordings_load_sinc_pcm(a.r->sinc.desc, a.d_src, a.r->bank.sampling_rate, table, entries, a.d_rows, a.stride,
                                                   a.r->bank.channels, a.stream));
    else
        SYLDET_HIP(launch_recordings_load_sinc(a.r->sinc.desc, a.d_src, a.s16, a.r->bank.sampling_rate, table, entries, a.d_rows, a.stride,
                                               a.r->bank.channels, a.stream));
    return SYLDET_OK;
}

int load_sinc_impl(syldet_recordings_t *r, const void *d_src, bool s16, const PcmSrc *pcm, const int64_t *src_offset, const int32_t *src_step,
                   const int64_t *src_samples, const double *src_rate, int32_t Z, double beta, double rho, float *d_rows,
                   int64_t channel_stride, hipStream_t stream)
{
    if (!r || !d_rows || (r->plan.K > 0 && (!d_src || !src_offset || !src_samples || !src_rate || (pcm && !pcm->format))))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int st = stride_arg(r, channel_stride)) return st;
    const Plan &p = r->plan;
    syldet_recordings::Sinc &s = r->sinc;
    const int K = p.K;
    const double rate = r->bank.sampling_rate;
    if (int st = source_args(K, src_offset, src_step)) return st;
    if (pcm)
        if (int st = pcm_args(K, d_src, *pcm, src_offset, src_step, [&](int k) { return src_samples[k]; })) return st;
    for (int k = 0; k < K; k++) {
        if (src_samples[k] < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "src_samples[" + std::to_string(k) + "] is negative");
        if (!(src_rate[k] > 0.0) || !std::isfinite(src_rate[k]))
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "src_rate[" + std::to_string(k) + "] is not a positive sampling rate");
    }
    if (int st = sinc_quality(Z, beta, rho)) return st;
    for (int k = 0; k < K; k++) {
        if (src_rate[k] != rate) {
            double sc = 0.0, H = 0.0;
            if (int st = sinc_design(src_rate[k], rate, Z, beta, rho, &sc, &H))
                return fail(st, std::string(syldet_last_error()) + " (recording " + std::to_string(k) + ")");
        }
        const int64_t n = syldet_convert_rate_count(src_samples[k], src_rate[k], rate);
        // (a copied recording reads its first n samples: n <= src_samples whatever the division rounds to)
        if (n != p.slots[(size_t)k].n_samples || (src_rate[k] == rate && n > src_samples[k]))
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "recording " + std::to_string(k) + " was planned with " + std::to_string(p.slots[(size_t)k].n_samples) +
                                                         " samples, but its " + std::to_string(src_samples[k]) + " source samples make " + std::to_string(n) +
                                                         " at the network's rate (syldet_convert_rate_count)");
    }
    if (p.row_samples == 0) return SYLDET_OK;
    // (a row's workgroups: one for every kSincBlockOut positions and at most one more a recording)
    if (p.row_samples / kSincBlockOut + K + 1 > 0x7fffffff) return fail(SYLDET_ERR_UNSUPPORTED, "rows too long for one launch of the converting load");
    // the key is the quality and the table itself: slot i holds the sources of recording order[i]
    RecSincDev *slots = (RecSincDev *)s.table.host.data();
    auto step = [&](int k) { return step_of(pcm, src_step, k); };
    bool same = s.table.kept && s.Z == Z && s.beta == beta && s.rho == rho;
    for (int i = 0; i < K && same; i++) {
        const int k = p.order[(size_t)i];
        same = slots[i].src_offset == src_offset[k] && slots[i].src_step == step(k) && slots[i].n_in == src_samples[k] && slots[i].rate_in == src_rate[k] &&
               slots[i].format == format_of(pcm, k);
    }
    SYLDET_HIP(hipSetDevice(r->bank.device));
    if (!same) {
        // new sources: the tables are re-made behind the last converting load that reads them
        int st = s.table.remake([&]() -> int {
            s.Z = Z; s.beta = beta; s.rho = rho;
            const int C = r->bank.channels;
            const int N = sinc_table_entries(Z);
            const std::vector<RecSlotDev> &table = r->load.table.host;   // (the plan's offsets and lengths, whatever its sources)
            int32_t *wg = (int32_t *)(s.table.host.data() + s.wg_at);
            int64_t grid = 0;
            for (int c = 0; c < C; c++) {
                const int sb = p.row_begin[(size_t)c], se = p.row_begin[(size_t)c + 1];
                int64_t at = 0;                                  // workgroups of the row so far
                for (int i = sb; i < se; i++) {
                    const int k = p.order[(size_t)i];
                    RecSincDev &d = slots[i];
                    d = RecSincDev{};
                    d.offset = table[(size_t)i].offset;
                    d.n_out = table[(size_t)i].n_samples;
                    d.span_end = i + 1 < se ? table[(size_t)i + 1].offset : p.row_samples;
                    d.src_offset = src_offset[k];
                    d.n_in = src_samples[k];
                    d.src_step = step(k);
                    d.format = (int16_t)format_of(pcm, k);
                    d.rate_in = src_rate[k];
                    d.copy = src_rate[k] == rate;
                    if (!d.copy) {
                        double sc = 0.0;
                        (void)sinc_design(src_rate[k], rate, Z, beta, rho, &sc, &d.H);    // (checked above)
                        d.scale = (float)sc;
                        d.idx_scale = (float)((double)N / d.H);  // as launch_sinc (kernels_sinc.hip) makes it
                    }
                    wg[i + c] = (int32_t)at;
                    at += (d.span_end - d.offset + kSincBlockOut - 1) / kSincBlockOut;
                }
                if (se > sb) wg[se + c] = (int32_t)at;
                else at = (p.row_samples + kSincBlockOut - 1) / kSincBlockOut;          // a row without a recording: +0
                grid = std::max(grid, at);
            }
            s.desc.grid_x = (int)grid;
            return SYLDET_OK;
        });
        if (st) return st;
    }
    s.table.read_on(stream);
    SincLaunch a{r, d_src, s16, pcm != nullptr, d_rows, channel_stride, stream};
    return sinc_table_use(Z, beta, sinc_launch, &a);
}

int plan_out(const Plan &p, syldet_slot_t *slots, int64_t *row_samples, int64_t *row_evals, double *fill)
{
    if (slots && p.K > 0) std::memcpy(slots, p.slots.data(), (size_t)p.K * sizeof(syldet_slot_t));
    if (row_samples) *row_samples = p.row_samples;
    if (row_evals) *row_evals = p.row_evals;
    if (fill) *fill = p.fill;
    return SYLDET_OK;
}

}  // namespace

extern "C" {

int syldet_recordings_plan(const syldet_t *h, const int64_t *n_samples, const int32_t *network, int32_t n_recordings,
                           syldet_slot_t *slots, int64_t *row_samples, int64_t *row_evals, double *fill)
{
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    Plan p;
    BankInfo b{};
    bank_info(h, &b);
    if (int st = make_plan(b, n_samples, network, n_recordings, p)) return st;
    return plan_out(p, slots, row_samples, row_evals, fill);
}

int syldet_recordings_plan_of_config(const syldet_config_t *cfg, int32_t n_channels, const int32_t *channel_net, const int64_t *n_samples,
                                     const int32_t *network, int32_t n_recordings, syldet_slot_t *slots, int64_t *row_samples,
                                     int64_t *row_evals, double *fill)
{
    if (!cfg || n_channels < 1) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL configuration or no channel");
    BankInfo b{};
    if (int st = compute_geometry(*cfg, &b.geom)) return st;
    b.channels = n_channels;
    b.sampling_rate = cfg->sampling_rate;
    b.window_length = cfg->window_length;
    b.time_range = cfg->time_range;
    std::vector<int> net;
    if (channel_net) {
        for (int32_t c = 0; c < n_channels; c++)
            if (channel_net[c] < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "channel_net[" + std::to_string(c) + "] is negative");
        net.assign(channel_net, channel_net + n_channels);
        b.channel_net = net.data();
    }
    Plan p;
    if (int st = make_plan(b, n_samples, network, n_recordings, p)) return st;
    return plan_out(p, slots, row_samples, row_evals, fill);
}

int syldet_recordings_create(const syldet_t *h, const int64_t *n_samples, const int32_t *network, int32_t n_recordings,
                             syldet_recordings_t **out)
{
    if (!out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    Plan plan;
    BankInfo b{};
    bank_info(h, &b);
    if (int st = make_plan(b, n_samples, network, n_recordings, plan)) return st;
    const int C = b.channels, K = plan.K, tiles = (int)((plan.row_samples + kRecTile - 1) / kRecTile);
    const RecBlob at((size_t)K, (size_t)C, (size_t)tiles);
    std::unique_ptr<syldet_recordings, int (*)(syldet_recordings_t *)> r(nullptr, syldet_recordings_destroy);
    std::vector<RecEventDev> events;
    std::vector<int32_t> tile_first;
    std::vector<int64_t> lengths;
    try {
        r.reset(new syldet_recordings());
        r->h = const_cast<syldet_t *>(h);
        r->bank = b;
        r->plan = std::move(plan);
        Plan &p = r->plan;
        std::vector<RecSlotDev> &table = r->load.table.host;
        p.order.resize((size_t)K);
        std::iota(p.order.begin(), p.order.end(), 0);
        // (row, offset), then the recordings without samples in front of one that shares their offset: the kernel takes the
        // LAST slot that starts at or before a position
        std::stable_sort(p.order.begin(), p.order.end(), [&](int32_t a, int32_t c) {
            const syldet_slot_t &x = p.slots[(size_t)a], &y = p.slots[(size_t)c];
            if (x.row != y.row) return x.row < y.row;
            if (x.offset != y.offset) return x.offset < y.offset;
            return x.n_samples < y.n_samples;
        });
        p.row_begin.assign((size_t)C + 1, 0);
        for (int32_t k : p.order) {
            const syldet_slot_t &s = p.slots[(size_t)k];
            table.push_back(RecSlotDev{s.offset, s.n_samples, 0, 1, 0});
            p.row_begin[(size_t)s.row + 1]++;
        }
        for (int c = 0; c < C; c++) p.row_begin[(size_t)c + 1] += p.row_begin[(size_t)c];
        tile_first.assign((size_t)C * (size_t)tiles, 0);
        for (int c = 0; c < C; c++) {
            int s = p.row_begin[(size_t)c];
            const int se = p.row_begin[(size_t)c + 1];
            for (int t = 0; t < tiles; t++) {
                while (s + 1 < se && table[(size_t)s + 1].offset <= (int64_t)t * kRecTile) s++;
                tile_first[(size_t)c * (size_t)tiles + (size_t)t] = s;
            }
        }
        for (const syldet_slot_t &s : p.slots) {
            events.push_back(RecEventDev{s.first_eval, s.n_evals, s.row, 0});
            lengths.push_back(s.n_samples);
        }
        // every table a call re-makes (each is its own key, too): room for them now, so that no call ever allocates
        r->sinc.table.host.assign(at.track - at.sinc, 0);
        r->tracks.layout.host.assign((size_t)K, RecTrackDev{});
        r->tracks.ls_begin.host.assign((size_t)K + 1, 0);
        r->levels.first.host.assign(2 * (size_t)K + 1, 0);
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    const Plan &p = r->plan;
    SYLDET_HIP(hipSetDevice(b.device));
    if (int st = r->blob.reserve(at.total)) return st;
    char *base = (char *)r->blob.ptr;
    // what never changes goes up now -- and the slots without sources: the track and level calls read their offsets and lengths,
    // and may come before any load
    auto upload = [&](size_t to, const auto &v) {
        return v.empty() ? hipSuccess : hipMemcpy(base + to, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice);
    };
    SYLDET_HIP(upload(at.table, r->load.table.host));
    SYLDET_HIP(upload(at.events, events));
    SYLDET_HIP(upload(at.row_begin, p.row_begin));
    SYLDET_HIP(upload(at.tile_first, tile_first));
    SYLDET_HIP(upload(at.n_samples, lengths));
    r->plan.d_events = (const RecEventDev *)(base + at.events);
    r->load.table.dev = (RecSlotDev *)(base + at.table);
    r->load.desc = RecLoadDesc{r->load.table.dev, (const int32_t *)(base + at.row_begin), (const int32_t *)(base + at.tile_first), tiles, p.row_samples};
    r->sinc.table.dev = base + at.sinc;
    r->sinc.wg_at = at.sinc_wg - at.sinc;
    r->sinc.desc = RecSincDesc{(const RecSincDev *)(base + at.sinc), r->load.desc.row_begin, (const int32_t *)(base + at.sinc_wg), 0, p.row_samples};
    r->tracks.layout.dev = (RecTrackDev *)(base + at.track);
    r->tracks.ls_begin.dev = (int32_t *)(base + at.ls_begin);
    r->tracks.desc = RecTrackDesc{r->load.desc, p.d_events, r->tracks.layout.dev, r->tracks.ls_begin.dev, (const int64_t *)(base + at.n_samples), K, p.row_evals};
    r->levels.first.dev = (int64_t *)(base + at.levels);
    r->levels.desc = RecLevelsDesc{r->load.desc, p.d_events, r->tracks.desc.n_samples, r->levels.first.dev, (const int64_t *)(base + at.slot_first), K,
                                   p.row_evals, 0};
    *out = r.release();
    return SYLDET_OK;
}

int syldet_recordings_destroy(syldet_recordings_t *r)
{
    if (!r) return SYLDET_OK;
    if (r->blob.ptr || r->tracks.last_seen.ptr) (void)hipSetDevice(r->bank.device);
    r->blob.release();
    r->tracks.last_seen.release();
    delete r;
    return SYLDET_OK;
}

int syldet_recordings_slots(const syldet_recordings_t *r, syldet_slot_t *slots)
{
    if (!r || (r->plan.K > 0 && !slots)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    return plan_out(r->plan, slots, nullptr, nullptr, nullptr);
}

int syldet_recordings_shape(const syldet_recordings_t *r, int32_t *n_recordings, int64_t *row_samples, int64_t *row_evals, double *fill)
{
    if (!r) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_recordings) *n_recordings = r->plan.K;
    return plan_out(r->plan, nullptr, row_samples, row_evals, fill);
}

int syldet_recordings_load_device(syldet_recordings_t *r, const float *d_src, const int64_t *src_offset, const int32_t *src_step,
                                  float *d_rows, int64_t channel_stride, void *hip_stream)
{
    return load_impl(r, d_src, false, nullptr, src_offset, src_step, d_rows, channel_stride, (hipStream_t)hip_stream);
}

int syldet_recordings_load_device_s16(syldet_recordings_t *r, const int16_t *d_src, const int64_t *src_offset, const int32_t *src_step,
                                      int16_t *d_rows, int64_t channel_stride, void *hip_stream)
{
    return load_impl(r, d_src, true, nullptr, src_offset, src_step, d_rows, channel_stride, (hipStream_t)hip_stream);
}

int syldet_recordings_load_sinc_device(syldet_recordings_t *r, const float *d_src, const int64_t *src_offset, const int32_t *src_step,
                                       const int64_t *src_samples, const double *src_rate, int32_t zero_crossings, double beta, double rolloff,
                                       float *d_rows, int64_t channel_stride, void *hip_stream)
{
    return load_sinc_impl(r, d_src, false, nullptr, src_offset, src_step, src_samples, src_rate, zero_crossings, beta, rolloff, d_rows, channel_stride,
                          (hipStream_t)hip_stream);
}

int syldet_recordings_load_sinc_device_s16(syldet_recordings_t *r, const int16_t *d_src, const int64_t *src_offset, const int32_t *src_step,
                                           const int64_t *src_samples, const double *src_rate, int32_t zero_crossings, double beta,
                                           double rolloff, float *d_rows, int64_t channel_stride, void *hip_stream)
{
    return load_sinc_impl(r, d_src, true, nullptr, src_offset, src_step, src_samples, src_rate, zero_crossings, beta, rolloff, d_rows, channel_stride,
                          (hipStream_t)hip_stream);
}

int syldet_recordings_load_pcm_device(syldet_recordings_t *r, const void *d_src, int64_t src_bytes, const int64_t *src_byte_offset,
                                      const int32_t *src_byte_step, const int32_t *src_format, float *d_rows, int64_t channel_stride,
                                      void *hip_stream)
{
    const PcmSrc pcm{src_bytes, src_format};
    return load_impl(r, d_src, false, &pcm, src_byte_offset, src_byte_step, d_rows, channel_stride, (hipStream_t)hip_stream);
}

int syldet_recordings_load_sinc_pcm_device(syldet_recordings_t *r, const void *d_src, int64_t src_bytes, const int64_t *src_byte_offset,
                                           const int32_t *src_byte_step, const int32_t *src_format, const int64_t *src_samples,
                                           const double *src_rate, int32_t zero_crossings, double beta, double rolloff, float *d_rows,
                                           int64_t channel_stride, void *hip_stream)
{
    const PcmSrc pcm{src_bytes, src_format};
    return load_sinc_impl(r, d_src, false, &pcm, src_byte_offset, src_byte_step, src_samples, src_rate, zero_crossings, beta, rolloff, d_rows,
                          channel_stride, (hipStream_t)hip_stream);
}

int syldet_recordings_events_device(syldet_recordings_t *r, const float *d_outputs, const uint8_t *d_flags, double debounce_seconds,
                                    int64_t *d_indices, float *d_values, int64_t capacity, int64_t *d_counts, void *hip_stream)
{
    if (!r || capacity < 0 || (capacity > 0 && !d_indices) || (r->plan.K > 0 && r->plan.row_evals > 0 && !d_flags) ||
        (d_outputs == nullptr) != (d_values == nullptr))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    if (r->plan.K == 0) return SYLDET_OK;
    SYLDET_HIP(hipSetDevice(r->bank.device));
    const int64_t debounce_frames = (int64_t)(debounce_seconds * r->bank.sampling_rate);   // TrackDetector.swift:19-26
    SYLDET_HIP(launch_recordings_events(r->plan.d_events, r->plan.K, r->plan.row_evals, r->bank.geom.outputs, d_outputs, d_flags, r->bank.geom.first_index,
                                        r->bank.geom.hop, debounce_frames, d_indices, d_values, capacity, d_counts, (hipStream_t)hip_stream));
    return SYLDET_OK;
}

}  // extern "C"
