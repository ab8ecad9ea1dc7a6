// syldet_recordings.cpp -- packed recordings (include/syldet.h, "packed recordings"): the plan that lays many recordings of
// different lengths end to end in a bank's rows, and the handle that keeps the plan's tables on the device so that the
// device calls (kernels_recordings.hip; kernels_recordings_sinc.hip for recordings at other rates) are launches only.  The handle
// itself is in syldet_recordings.hpp; its per-sample tracks are in syldet_recordings_tracks.cpp,
// its level meters in syldet_recordings_levels.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "syldet_recordings.hpp"

using sd::fail;

namespace {

struct Plan {
    std::vector<syldet_slot_t> slots;
    int64_t row_samples = 0, row_evals = 0;
    double fill = 0.0;
};

// syldet_count_evals from the clock alone (count_evals of syldet_api.cpp)
int64_t evals_of(const sd::BankInfo &b, int64_t S)
{
    const int64_t need = (int64_t)b.geom.gap + b.window_length;
    const int64_t J = S < need ? 0 : (S - need) / b.geom.hop + 1;
    return J >= b.time_range ? J - b.time_range + 1 : 0;
}

// b: the bank's clock, channels and channel_net (a handle's, or a configuration's: no device either way)
int make_plan(const sd::BankInfo &b, const int64_t *n_samples, const int32_t *network, int32_t K, Plan &p)
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
            s.n_evals = evals_of(b, n_samples[k]);
            s.n_samples = n_samples[k];
            fills[(size_t)best] += padded[(size_t)k];
            total += (double)n_samples[k];
        }
        const int64_t most = C > 0 && K > 0 ? *std::max_element(fills.begin(), fills.end()) : 0;
        p.row_samples = (most + 7) / 8 * 8;
        p.row_evals = evals_of(b, p.row_samples);
        p.fill = p.row_samples > 0 ? total / ((double)C * (double)p.row_samples) : 0.0;
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    return SYLDET_OK;
}

size_t up16(size_t n) { return (n + 15) / 16 * 16; }

int load_impl(syldet_recordings_t *r, const void *d_src, bool s16, const int64_t *src_offset, const int32_t *src_step, void *d_rows,
              int64_t channel_stride, hipStream_t stream)
{
    if (!r || !d_rows || (r->K > 0 && (!d_src || !src_offset))) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (channel_stride < r->row_samples) return fail(SYLDET_ERR_INVALID_ARGUMENT, "channel_stride below row_samples");
    bool same = !r->src_offset.empty() || r->K == 0;
    for (int k = 0; k < r->K; k++) {
        const int32_t step = src_step ? src_step[k] : 1;
        if (src_offset[k] < 0 || step < 1) return fail(SYLDET_ERR_INVALID_ARGUMENT, "a negative source offset or a step below 1 (recording " + std::to_string(k) + ")");
        same = same && r->src_offset[(size_t)k] == src_offset[k] && r->src_step[(size_t)k] == step;
    }
    if (r->row_samples == 0) return SYLDET_OK;
    SYLDET_HIP(hipSetDevice(r->bank.device));
    if (!same) {
        // new sources: the table is re-made behind the last load that reads it (the one copy the header speaks of)
        if (!r->src_offset.empty()) SYLDET_HIP(hipStreamSynchronize(r->last_load));
        try {
            r->src_offset.assign(src_offset, src_offset + r->K);
            r->src_step.assign((size_t)r->K, 1);
            if (src_step) r->src_step.assign(src_step, src_step + r->K);
        } catch (const std::bad_alloc &) {
            return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
        }
        for (size_t i = 0; i < r->table.size(); i++) {
            r->table[i].src_offset = r->src_offset[(size_t)r->order[i]];
            r->table[i].src_step = r->src_step[(size_t)r->order[i]];
        }
        hipError_t e = hipMemcpy(r->d_blob, r->table.data(), r->table.size() * sizeof(sd::RecSlotDev), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            r->src_offset.clear();
            return fail(SYLDET_ERR_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(e));
        }
    }
    r->last_load = stream;
    SYLDET_HIP(sd::launch_recordings_load(r->load, d_src, s16, d_rows, channel_stride, r->bank.channels, stream));
    return SYLDET_OK;
}

// ---- the converting load: recordings at other rates brought to the network's as the rows load ----
struct SincLaunch {
    syldet_recordings_t *r;
    const void *d_src;
    bool s16;
    float *d_rows;
    int64_t stride;
    hipStream_t stream;
};

int sinc_launch(const float *table, int entries, void *ctx)
{
    const SincLaunch &a = *(const SincLaunch *)ctx;
    SYLDET_HIP(sd::launch_recordings_load_sinc(a.r->sinc, a.d_src, a.s16, a.r->bank.sampling_rate, table, entries, a.d_rows, a.stride,
                                               a.r->bank.channels, a.stream));
    return SYLDET_OK;
}

int load_sinc_impl(syldet_recordings_t *r, const void *d_src, bool s16, const int64_t *src_offset, const int32_t *src_step,
                   const int64_t *src_samples, const double *src_rate, int32_t Z, double beta, double rho, float *d_rows,
                   int64_t channel_stride, hipStream_t stream)
{
    if (!r || !d_rows || (r->K > 0 && (!d_src || !src_offset || !src_samples || !src_rate))) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (channel_stride < r->row_samples) return fail(SYLDET_ERR_INVALID_ARGUMENT, "channel_stride below row_samples");
    const int K = r->K;
    const double rate = r->bank.sampling_rate;
    for (int k = 0; k < K; k++) {
        const int32_t step = src_step ? src_step[k] : 1;
        if (src_offset[k] < 0 || step < 1) return fail(SYLDET_ERR_INVALID_ARGUMENT, "a negative source offset or a step below 1 (recording " + std::to_string(k) + ")");
    }
    for (int k = 0; k < K; k++) {
        if (src_samples[k] < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "src_samples[" + std::to_string(k) + "] is negative");
        if (!(src_rate[k] > 0.0) || !std::isfinite(src_rate[k]))
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "src_rate[" + std::to_string(k) + "] is not a positive sampling rate");
    }
    if (int st = sd::sinc_quality(Z, beta, rho)) return st;
    bool same = r->sinc_kept && r->sinc_Z == Z && r->sinc_beta == beta && r->sinc_rho == rho;
    for (int k = 0; k < K; k++) {
        if (src_rate[k] != rate) {
            double s = 0.0, H = 0.0;
            if (int st = sd::sinc_design(src_rate[k], rate, Z, beta, rho, &s, &H))
                return fail(st, std::string(syldet_last_error()) + " (recording " + std::to_string(k) + ")");
        }
        const int64_t n = syldet_convert_rate_count(src_samples[k], src_rate[k], rate);
        // (a copied recording reads its first n samples: n <= src_samples whatever the division rounds to)
        if (n != r->slots[(size_t)k].n_samples || (src_rate[k] == rate && n > src_samples[k]))
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "recording " + std::to_string(k) + " was planned with " + std::to_string(r->slots[(size_t)k].n_samples) +
                                                         " samples, but its " + std::to_string(src_samples[k]) + " source samples make " + std::to_string(n) +
                                                         " at the network's rate (syldet_convert_rate_count)");
        same = same && r->sinc_offset[(size_t)k] == src_offset[k] && r->sinc_step[(size_t)k] == (src_step ? src_step[k] : 1) &&
               r->sinc_samples[(size_t)k] == src_samples[k] && r->sinc_rate[(size_t)k] == src_rate[k];
    }
    if (r->row_samples == 0) return SYLDET_OK;
    // (a row's workgroups: one for every kSincBlockOut positions and at most one more a recording)
    if (r->row_samples / sd::kSincBlockOut + K + 1 > 0x7fffffff) return fail(SYLDET_ERR_UNSUPPORTED, "rows too long for one launch of the converting load");
    SYLDET_HIP(hipSetDevice(r->bank.device));
    if (!same) {
        // new sources: the tables are re-made behind the last converting load that reads them (the one copy the header speaks of)
        if (r->sinc_kept) SYLDET_HIP(hipStreamSynchronize(r->sinc_last_load));
        r->sinc_kept = false;
        r->sinc_offset.assign(src_offset, src_offset + K);   // (reserved by syldet_recordings_create: no allocation)
        r->sinc_step.assign((size_t)K, 1);
        if (src_step) r->sinc_step.assign(src_step, src_step + K);
        r->sinc_samples.assign(src_samples, src_samples + K);
        r->sinc_rate.assign(src_rate, src_rate + K);
        r->sinc_Z = Z; r->sinc_beta = beta; r->sinc_rho = rho;
        const int C = r->bank.channels;
        const int N = sd::sinc_table_entries(Z);
        sd::RecSincDev *slots = (sd::RecSincDev *)r->sinc_host.data();
        int32_t *wg = (int32_t *)(r->sinc_host.data() + r->sinc_wg_at);
        int64_t grid = 0;
        for (int c = 0; c < C; c++) {
            const int sb = r->row_begin[(size_t)c], se = r->row_begin[(size_t)c + 1];
            int64_t at = 0;                                  // workgroups of the row so far
            for (int i = sb; i < se; i++) {
                const int k = r->order[(size_t)i];
                sd::RecSincDev &d = slots[i];
                d = sd::RecSincDev{};
                d.offset = r->table[(size_t)i].offset;
                d.n_out = r->table[(size_t)i].n_samples;
                d.span_end = i + 1 < se ? r->table[(size_t)i + 1].offset : r->row_samples;
                d.src_offset = src_offset[k];
                d.n_in = src_samples[k];
                d.src_step = src_step ? src_step[k] : 1;
                d.rate_in = src_rate[k];
                d.copy = src_rate[k] == rate;
                if (!d.copy) {
                    double s = 0.0;
                    (void)sd::sinc_design(src_rate[k], rate, Z, beta, rho, &s, &d.H);    // (checked above)
                    d.scale = (float)s;
                    d.idx_scale = (float)((double)N / d.H);  // as launch_sinc (kernels_sinc.hip) makes it
                }
                wg[i + c] = (int32_t)at;
                at += (d.span_end - d.offset + sd::kSincBlockOut - 1) / sd::kSincBlockOut;
            }
            if (se > sb) wg[se + c] = (int32_t)at;
            else at = (r->row_samples + sd::kSincBlockOut - 1) / sd::kSincBlockOut;      // a row without a recording: +0
            grid = std::max(grid, at);
        }
        r->sinc.grid_x = (int)grid;
        hipError_t e = hipMemcpy(r->d_sinc, r->sinc_host.data(), r->sinc_host.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(SYLDET_ERR_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(e));
        r->sinc_kept = true;
    }
    r->sinc_last_load = stream;
    SincLaunch a{r, d_src, s16, d_rows, channel_stride, stream};
    return sd::sinc_table_use(Z, beta, sinc_launch, &a);
}

}  // namespace

extern "C" {

static int plan_out(const Plan &p, int32_t K, syldet_slot_t *slots, int64_t *row_samples, int64_t *row_evals, double *fill)
{
    if (slots && K > 0) std::memcpy(slots, p.slots.data(), (size_t)K * sizeof(syldet_slot_t));
    if (row_samples) *row_samples = p.row_samples;
    if (row_evals) *row_evals = p.row_evals;
    if (fill) *fill = p.fill;
    return SYLDET_OK;
}

int syldet_recordings_plan(const syldet_t *h, const int64_t *n_samples, const int32_t *network, int32_t n_recordings,
                           syldet_slot_t *slots, int64_t *row_samples, int64_t *row_evals, double *fill)
{
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    Plan p;
    sd::BankInfo b{};
    sd::bank_info(h, &b);
    if (int st = make_plan(b, n_samples, network, n_recordings, p)) return st;
    return plan_out(p, n_recordings, slots, row_samples, row_evals, fill);
}

int syldet_recordings_plan_of_config(const syldet_config_t *cfg, int32_t n_channels, const int32_t *channel_net, const int64_t *n_samples,
                                     const int32_t *network, int32_t n_recordings, syldet_slot_t *slots, int64_t *row_samples,
                                     int64_t *row_evals, double *fill)
{
    if (!cfg || n_channels < 1) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL configuration or no channel");
    sd::BankInfo b{};
    if (int st = sd::compute_geometry(*cfg, &b.geom)) return st;
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
    return plan_out(p, n_recordings, slots, row_samples, row_evals, fill);
}

int syldet_recordings_create(const syldet_t *h, const int64_t *n_samples, const int32_t *network, int32_t n_recordings,
                             syldet_recordings_t **out)
{
    if (!out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    Plan p;
    sd::BankInfo b{};
    sd::bank_info(h, &b);
    if (int st = make_plan(b, n_samples, network, n_recordings, p)) return st;
    std::unique_ptr<syldet_recordings, int (*)(syldet_recordings_t *)> r(nullptr, syldet_recordings_destroy);
    std::vector<sd::RecEventDev> events;
    std::vector<int32_t> row_begin, tile_first;
    std::vector<int64_t> lengths;
    int tiles = 0;
    try {
        r.reset(new syldet_recordings());
        r->h = const_cast<syldet_t *>(h);
        r->bank = b;
        r->K = n_recordings;
        r->slots = std::move(p.slots);
        r->row_samples = p.row_samples;
        r->row_evals = p.row_evals;
        r->fill = p.fill;
        const int C = b.channels, K = r->K;
        r->order.resize((size_t)K);
        std::iota(r->order.begin(), r->order.end(), 0);
        // (row, offset), then the recordings without samples in front of one that shares their offset: the kernel takes the
        // LAST slot that starts at or before a position
        std::stable_sort(r->order.begin(), r->order.end(), [&](int32_t a, int32_t c) {
            const syldet_slot_t &x = r->slots[(size_t)a], &y = r->slots[(size_t)c];
            if (x.row != y.row) return x.row < y.row;
            if (x.offset != y.offset) return x.offset < y.offset;
            return x.n_samples < y.n_samples;
        });
        row_begin.assign((size_t)C + 1, 0);
        for (int32_t k : r->order) {
            const syldet_slot_t &s = r->slots[(size_t)k];
            r->table.push_back(sd::RecSlotDev{s.offset, s.n_samples, 0, 1, 0});
            row_begin[(size_t)s.row + 1]++;
        }
        for (int c = 0; c < C; c++) row_begin[(size_t)c + 1] += row_begin[(size_t)c];
        tiles = (int)((r->row_samples + sd::kRecTile - 1) / sd::kRecTile);
        tile_first.assign((size_t)C * (size_t)tiles, 0);
        for (int c = 0; c < C; c++) {
            int s = row_begin[(size_t)c];
            const int se = row_begin[(size_t)c + 1];
            for (int t = 0; t < tiles; t++) {
                while (s + 1 < se && r->table[(size_t)s + 1].offset <= (int64_t)t * sd::kRecTile) s++;
                tile_first[(size_t)c * (size_t)tiles + (size_t)t] = s;
            }
        }
        for (int k = 0; k < K; k++) events.push_back(sd::RecEventDev{r->slots[(size_t)k].first_eval, r->slots[(size_t)k].n_evals, r->slots[(size_t)k].row, 0});
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    const size_t n_table = up16(r->table.size() * sizeof(sd::RecSlotDev)), n_events = up16(events.size() * sizeof(sd::RecEventDev)),
                 n_begin = up16(row_begin.size() * sizeof(int32_t)), n_tiles = up16(tile_first.size() * sizeof(int32_t));
    // the converting load's tables, K + C words: room for them now, so that no load ever allocates
    r->sinc_wg_at = up16(r->table.size() * sizeof(sd::RecSincDev));
    const size_t n_sinc = r->sinc_wg_at + up16((r->table.size() + (size_t)b.channels) * sizeof(int32_t));
    try {
        r->row_begin = row_begin;
        r->sinc_host.assign(n_sinc, 0);
        r->sinc_offset.reserve((size_t)r->K);
        r->sinc_samples.reserve((size_t)r->K);
        r->sinc_step.reserve((size_t)r->K);
        r->sinc_rate.reserve((size_t)r->K);
        // the tracks' tables likewise
        r->track_offset.reserve((size_t)r->K);
        r->track_step.reserve((size_t)r->K);
        r->track_host.assign((size_t)r->K, sd::RecTrackDev{});
        r->ls_host.assign((size_t)r->K + 1, 0);
        // ... and the level meters'
        r->levels_host.assign(2 * (size_t)r->K + 1, 0);
        for (int k = 0; k < r->K; k++) lengths.push_back(r->slots[(size_t)k].n_samples);
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    // ... and the tracks': destinations [K] | last_seen prefix [K + 1] | lengths [K]
    const size_t n_track = up16(r->table.size() * sizeof(sd::RecTrackDev)), n_ls = up16((r->table.size() + 1) * sizeof(int32_t)),
                 n_len = up16(r->table.size() * sizeof(int64_t));
    // ... and the level meters': reading_first [K + 1] | slot_first [K]
    const size_t n_levels = up16((2 * r->table.size() + 1) * sizeof(int64_t));
    SYLDET_HIP(hipSetDevice(b.device));
    hipError_t e = hipMalloc(&r->d_blob, n_table + n_events + n_begin + n_tiles + n_sinc + n_track + n_ls + n_len + n_levels + 16);
    if (e != hipSuccess) {
        r->d_blob = nullptr;
        return fail(e == hipErrorOutOfMemory ? SYLDET_ERR_OUT_OF_MEMORY : SYLDET_ERR_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    char *base = (char *)r->d_blob;
    // (the slots without sources: the track calls read their offsets and lengths, and may come before any load)
    if (!r->table.empty()) SYLDET_HIP(hipMemcpy(base, r->table.data(), r->table.size() * sizeof(sd::RecSlotDev), hipMemcpyHostToDevice));
    if (!events.empty()) SYLDET_HIP(hipMemcpy(base + n_table, events.data(), events.size() * sizeof(sd::RecEventDev), hipMemcpyHostToDevice));
    SYLDET_HIP(hipMemcpy(base + n_table + n_events, row_begin.data(), row_begin.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!tile_first.empty()) SYLDET_HIP(hipMemcpy(base + n_table + n_events + n_begin, tile_first.data(), tile_first.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    r->load = sd::RecLoadDesc{(const sd::RecSlotDev *)base, (const int32_t *)(base + n_table + n_events),
                              (const int32_t *)(base + n_table + n_events + n_begin), tiles, r->row_samples};
    r->d_events = (const sd::RecEventDev *)(base + n_table);
    r->d_sinc = base + n_table + n_events + n_begin + n_tiles;
    r->sinc = sd::RecSincDesc{(const sd::RecSincDev *)r->d_sinc, r->load.row_begin, (const int32_t *)(r->d_sinc + r->sinc_wg_at), 0, r->row_samples};
    char *tracks = r->d_sinc + n_sinc;
    r->d_track = (sd::RecTrackDev *)tracks;
    r->d_ls_begin = (int32_t *)(tracks + n_track);
    if (!lengths.empty()) SYLDET_HIP(hipMemcpy(tracks + n_track + n_ls, lengths.data(), lengths.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    r->track = sd::RecTrackDesc{r->load, r->d_events, r->d_track, r->d_ls_begin, (const int64_t *)(tracks + n_track + n_ls), r->K, r->row_evals};
    r->d_levels_first = (int64_t *)(tracks + n_track + n_ls + n_len);
    r->levels = sd::RecLevelsDesc{r->load, r->d_events, r->track.n_samples, r->d_levels_first, r->d_levels_first + r->K + 1, r->K, r->row_evals, 0};
    *out = r.release();
    return SYLDET_OK;
}

int syldet_recordings_destroy(syldet_recordings_t *r)
{
    if (!r) return SYLDET_OK;
    if (r->d_blob) {
        (void)hipSetDevice(r->bank.device);
        (void)hipFree(r->d_blob);
    }
    if (r->d_last_seen) {
        (void)hipSetDevice(r->bank.device);
        (void)hipFree(r->d_last_seen);
    }
    delete r;
    return SYLDET_OK;
}

int syldet_recordings_slots(const syldet_recordings_t *r, syldet_slot_t *slots)
{
    if (!r || (r->K > 0 && !slots)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (r->K > 0) std::memcpy(slots, r->slots.data(), (size_t)r->K * sizeof(syldet_slot_t));
    return SYLDET_OK;
}

int syldet_recordings_shape(const syldet_recordings_t *r, int32_t *n_recordings, int64_t *row_samples, int64_t *row_evals, double *fill)
{
    if (!r) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_recordings) *n_recordings = r->K;
    if (row_samples) *row_samples = r->row_samples;
    if (row_evals) *row_evals = r->row_evals;
    if (fill) *fill = r->fill;
    return SYLDET_OK;
}

int syldet_recordings_load_device(syldet_recordings_t *r, const float *d_src, const int64_t *src_offset, const int32_t *src_step,
                                  float *d_rows, int64_t channel_stride, void *hip_stream)
{
    return load_impl(r, d_src, false, src_offset, src_step, d_rows, channel_stride, (hipStream_t)hip_stream);
}

int syldet_recordings_load_device_s16(syldet_recordings_t *r, const int16_t *d_src, const int64_t *src_offset, const int32_t *src_step,
                                      int16_t *d_rows, int64_t channel_stride, void *hip_stream)
{
    return load_impl(r, d_src, true, src_offset, src_step, d_rows, channel_stride, (hipStream_t)hip_stream);
}

int syldet_recordings_load_sinc_device(syldet_recordings_t *r, const float *d_src, const int64_t *src_offset, const int32_t *src_step,
                                       const int64_t *src_samples, const double *src_rate, int32_t zero_crossings, double beta, double rolloff,
                                       float *d_rows, int64_t channel_stride, void *hip_stream)
{
    return load_sinc_impl(r, d_src, false, src_offset, src_step, src_samples, src_rate, zero_crossings, beta, rolloff, d_rows, channel_stride,
                          (hipStream_t)hip_stream);
}

int syldet_recordings_load_sinc_device_s16(syldet_recordings_t *r, const int16_t *d_src, const int64_t *src_offset, const int32_t *src_step,
                                           const int64_t *src_samples, const double *src_rate, int32_t zero_crossings, double beta,
                                           double rolloff, float *d_rows, int64_t channel_stride, void *hip_stream)
{
    return load_sinc_impl(r, d_src, true, src_offset, src_step, src_samples, src_rate, zero_crossings, beta, rolloff, d_rows, channel_stride,
                          (hipStream_t)hip_stream);
}

int syldet_recordings_events_device(syldet_recordings_t *r, const float *d_outputs, const uint8_t *d_flags, double debounce_seconds,
                                    int64_t *d_indices, float *d_values, int64_t capacity, int64_t *d_counts, void *hip_stream)
{
    if (!r || capacity < 0 || (capacity > 0 && !d_indices) || (r->K > 0 && r->row_evals > 0 && !d_flags) || (d_outputs == nullptr) != (d_values == nullptr))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    if (r->K == 0) return SYLDET_OK;
    SYLDET_HIP(hipSetDevice(r->bank.device));
    const int64_t debounce_frames = (int64_t)(debounce_seconds * r->bank.sampling_rate);   // TrackDetector.swift:19-26
    SYLDET_HIP(sd::launch_recordings_events(r->d_events, r->K, r->row_evals, r->bank.geom.outputs, d_outputs, d_flags, r->bank.geom.first_index,
                                            r->bank.geom.hop, debounce_frames, d_indices, d_values, capacity, d_counts, (hipStream_t)hip_stream));
    return SYLDET_OK;
}

}  // extern "C"
