// The batch path (--batch, see BatchOpt): consecutive audio files through one bank, stage by stage over one state.
#pragma once

#include "one_file.hpp"

namespace {

struct BatchFile {
    std::string path;
    wav::Info info;
    std::vector<unsigned char> raw;                         // the frames as the file's data chunk stores them (wav::read_raw)
    bool is16 = false;
    bool convert = false;                                   // at another rate than the network's: converted as the rows load (--resample sinc)
    // what --batch counts: the bytes of the rows the file's samples make at its own rate (int16 rows for a 16-bit file, else fp32)
    size_t bytes() const { return (size_t)info.frames * (size_t)info.channels * (is16 ? sizeof(int16_t) : sizeof(float)); }
    int sample_bytes() const { return info.bits / 8; }
    int32_t format() const                                  // SYLDET_PCM_* of the file's samples
    {
        if (info.format == 3) return info.bits == 32 ? SYLDET_PCM_F32 : SYLDET_PCM_F64;
        return info.bits == 8 ? SYLDET_PCM_U8 : info.bits == 16 ? SYLDET_PCM_S16 : info.bits == 24 ? SYLDET_PCM_S24 : SYLDET_PCM_S32;
    }
};

// Where a batch's files lie: every track of every file is a recording, in the files' order
struct BatchPlan {
    bool all16 = true, converting = false;
    size_t el = 1;                                          // the unit of the source's offsets and steps: int16 elements, or bytes
    int32_t K = 0;                                          // recordings
    // the source: the upload, and recording k's samples in it
    std::vector<int64_t> file_at;                           // where a file's frames lie in the upload, in that unit (whole 16 bytes)
    std::vector<int64_t> lengths, src_offset, src_samples;
    std::vector<double> src_rate;
    std::vector<int32_t> network, src_step, src_format;
    int64_t total = 0;
    // the tracks' destination: file i's frames [n_i][tracks] at frames_at[i], n_i its length at the network's rate
    std::vector<int64_t> dst_offset, frames_at;
    std::vector<int32_t> dst_step;
    int64_t dst_total = 0;
};

// Stage 1, host arithmetic only.
// A batch that holds a file at another rate: every recording is planned with its length at the network's rate and loaded
// through the converting load (syldet_recordings_load_sinc_device_s16, syldet_recordings_load_sinc_pcm_device: the files at the
// network's rate are copied), fp32 rows.
// The upload is the files' data chunks as they are stored.  A batch of 16-bit files is an int16 array (int16 rows, as ever);
// any other batch is bytes, every file in its own sample format, decoded as the rows load (syldet_recordings_load_pcm_device):
// no sample is converted on the host.
BatchPlan plan_batch(const std::vector<BatchFile> &files, double rate)
{
    BatchPlan p;
    for (const BatchFile &f : files) {
        p.all16 = p.all16 && f.is16;
        p.converting = p.converting || f.convert;
    }
    p.el = p.all16 ? sizeof(int16_t) : 1;
    const int64_t align = (int64_t)(16 / p.el);
    for (const BatchFile &f : files) {
        const int tracks = f.info.channels;
        const int64_t sample = p.all16 ? 1 : f.sample_bytes();
        const int64_t length = p.converting ? syldet_convert_rate_count(f.info.frames, f.info.rate, rate) : f.info.frames;
        p.file_at.push_back(p.total);
        p.frames_at.push_back(p.dst_total);
        for (int t = 0; t < tracks; t++) {
            p.lengths.push_back(length);
            p.src_samples.push_back(f.info.frames);
            p.src_rate.push_back(f.info.rate);
            p.network.push_back(t);
            p.src_offset.push_back(p.total + t * sample);
            p.src_step.push_back((int32_t)(tracks * sample));
            p.src_format.push_back(f.format());
            p.dst_offset.push_back(p.dst_total + t);
            p.dst_step.push_back(tracks);
        }
        p.total += ((int64_t)(f.raw.size() / p.el) + align - 1) / align * align;
        p.dst_total += (length * tracks + 7) / 8 * 8;
    }
    p.K = (int32_t)p.lengths.size();
    return p;
}

struct Batch {
    const Run &run;
    const std::vector<BatchFile> &files;
    const BatchPlan plan;
    const syldet_config_t *cfg;
    // the bank
    int C = 0, n_out = 0;
    syldet_t *h = nullptr;
    syldet_recordings_t *r = nullptr;
    hipStream_t stream = nullptr;
    int64_t row_samples = 0, row_evals = 0;
    bool ran = false;                                       // a file of the batch has an evaluation
    int st = 0;                                             // what the scorer left: the windows and the tracks behind it go by it
    // what comes back: the detections ...
    std::vector<int64_t> idx, cnt;
    std::vector<float> val;
    int64_t cap = 1;
    // ... the tracks (zeros where no file of the batch has an evaluation) ...
    std::vector<int16_t> sim_frames, ttl_frames;
    std::vector<int64_t> on_idx, on_cnt;
    int64_t on_cap = 1;
    // ... --levels-dir: the two tables of every recording, flat as syldet_recordings_levels_layout lays them, and which readings have
    // no evaluation ...
    int64_t lv_P = 1;
    std::vector<int64_t> lv_first;
    std::vector<double> lv_in;
    std::vector<float> lv_out;
    std::vector<uint8_t> lv_empty;
    // ... --align-dir: every recording's events, their windows (recording k's from al.begin[k]), and what decides presence
    Aligned al;
    // ... --match: every recording's matches
    std::vector<std::vector<int64_t>> matched;
    // --score: the recordings' labels in the recordings' order
    std::vector<int64_t> score_labels, score_begin{0};
};

// ... and what it holds on the device while it runs
struct BatchDevice {
    DevBuf d_src, d_rows, d_out, d_flags, d_idx, d_val, d_cnt, d_al_rows, d_al_cols, d_lv_in, d_lv_out;
};

// Stage 2: the bank and its plan; the upload, the load into the rows and the run.  0, 2, or -1: nothing of the batch needs the device.
int load_and_run(Batch &b, BatchDevice &d)
{
    const BatchPlan &p = b.plan;
    const Run &run = b.run;
    const ResampleOpt &conv = run.opt.conv;
    const int n_nets = (int)run.cfgs.size(), C = b.C;
    std::vector<int32_t> row_net((size_t)C);
    for (int c = 0; c < C; c++) row_net[(size_t)c] = c % n_nets;
    if (int st = n_nets > 1 ? syldet_create_mixed(run.cfgs.data(), n_nets, row_net.data(), C, run.opt.device, SYLDET_ENGINE_AUTO, &b.h)
                            : syldet_create(b.cfg, C, run.opt.device, SYLDET_ENGINE_AUTO, &b.h)) {
        std::fprintf(stderr, "Unable to create the detector: %s: %s\n", syldet_strerror(st), syldet_last_error());
        return 2;
    }
    syldet_geometry_t g;
    syldet_get_geometry(b.h, &g);
    b.n_out = g.outputs;
    int st = syldet_recordings_create(b.h, p.lengths.data(), n_nets > 1 ? p.network.data() : nullptr, p.K, &b.r);
    if (!st) st = syldet_recordings_shape(b.r, nullptr, &b.row_samples, &b.row_evals, nullptr);
    if (st) {
        std::fprintf(stderr, "Unable to plan the batch: %s: %s\n", syldet_strerror(st), syldet_last_error());
        return 2;
    }
    const bool ran = b.ran = b.row_evals > 0;
    const int64_t rs = b.row_samples;
    if (!ran && run.opt.dirs.levels.empty() && !run.align && !run.match) return -1;   // every file shorter than one evaluation: no events (the input meter reads them all the same)
    if (hipSetDevice(run.opt.device) != hipSuccess || hipStreamCreate(&b.stream) != hipSuccess) return 2;
    if (!d.d_src.alloc((size_t)p.total * p.el) || !d.d_rows.alloc((size_t)C * rs * (p.converting || !p.all16 ? sizeof(float) : sizeof(int16_t))) ||
        !d.d_out.alloc((size_t)C * b.row_evals * b.n_out * sizeof(float)) || !d.d_flags.alloc((size_t)C * b.row_evals) || !d.d_cnt.alloc((size_t)p.K * sizeof(int64_t))) return 2;
    for (size_t i = 0; i < b.files.size(); i++)
        if (hipMemcpyAsync((char *)d.d_src.p + (size_t)p.file_at[i] * p.el, b.files[i].raw.data(), b.files[i].raw.size(), hipMemcpyHostToDevice, b.stream) != hipSuccess) return 2;
    if (p.converting) {
        st = p.all16 ? syldet_recordings_load_sinc_device_s16(b.r, (const int16_t *)d.d_src.p, p.src_offset.data(), p.src_step.data(), p.src_samples.data(), p.src_rate.data(),
                                                              conv.zero_crossings, conv.beta, conv.rolloff, (float *)d.d_rows.p, rs, b.stream)
                     : syldet_recordings_load_sinc_pcm_device(b.r, d.d_src.p, p.total, p.src_offset.data(), p.src_step.data(), p.src_format.data(), p.src_samples.data(),
                                                              p.src_rate.data(), conv.zero_crossings, conv.beta, conv.rolloff, (float *)d.d_rows.p, rs, b.stream);
    } else if (p.all16) {
        st = syldet_recordings_load_device_s16(b.r, (const int16_t *)d.d_src.p, p.src_offset.data(), p.src_step.data(), (int16_t *)d.d_rows.p, rs, b.stream);
    } else {
        st = syldet_recordings_load_pcm_device(b.r, d.d_src.p, p.total, p.src_offset.data(), p.src_step.data(), p.src_format.data(), (float *)d.d_rows.p, rs, b.stream);
    }
    if (!st && ran && p.all16 && !p.converting) st = syldet_run_device_s16(b.h, (const int16_t *)d.d_rows.p, rs, rs, (float *)d.d_out.p, (uint8_t *)d.d_flags.p, b.stream);
    else if (!st && ran) st = syldet_run_device(b.h, (const float *)d.d_rows.p, rs, rs, (float *)d.d_out.p, (uint8_t *)d.d_flags.p, b.stream);
    if (st) std::fprintf(stderr, "Unable to process the batch: %s: %s\n", syldet_strerror(st), syldet_last_error());
    return st ? 2 : 0;
}

// Stage 3: the level tables of every file of the batch: the input meter on the very rows that are run (int16 rows for 16-bit files, fp32
// rows for float files and for converted ones), the output meter on the outputs the run left; only the two tables come back
int batch_meters(Batch &b, BatchDevice &d)
{
    const LevelsOpt &levels = b.run.opt.levels;
    const int32_t K = b.plan.K;
    if (b.run.opt.dirs.levels.empty()) return 0;
    int64_t n_readings = 0;
    std::vector<syldet_slot_t> slots((size_t)std::max<int32_t>(K, 1));
    int st = syldet_recordings_levels_layout(b.r, levels.buffer, b.lv_P, b.lv_first.data(), &n_readings);
    if (!st) st = syldet_recordings_slots(b.r, slots.data());
    if (!st) {
        b.lv_in.assign((size_t)n_readings, 0.0);
        b.lv_out.assign((size_t)n_readings, 0.0f);
        b.lv_empty.assign((size_t)n_readings, 1);
        for (int32_t k = 0; k < K; k++)
            for (int64_t m = 0; m < b.lv_first[(size_t)k + 1] - b.lv_first[(size_t)k]; m++) {
                int64_t first = 0, count = 0;
                if (syldet_levels_eval_range(b.h, slots[(size_t)k].n_samples, slots[(size_t)k].n_evals, levels.buffer, b.lv_P, m, &first, &count) == SYLDET_OK)
                    b.lv_empty[(size_t)(b.lv_first[(size_t)k] + m)] = count == 0;
            }
        if (!d.d_lv_in.alloc((size_t)n_readings * sizeof(double)) || !d.d_lv_out.alloc((size_t)n_readings * sizeof(float))) return 2;
    }
    if (!st && n_readings > 0) {
        st = b.plan.all16 && !b.plan.converting ? syldet_recordings_levels_device_s16(b.r, (const int16_t *)d.d_rows.p, b.row_samples, levels.buffer, b.lv_P, (double *)d.d_lv_in.p, n_readings, b.stream)
                                                : syldet_recordings_levels_device(b.r, (const float *)d.d_rows.p, b.row_samples, levels.buffer, b.lv_P, (double *)d.d_lv_in.p, n_readings, b.stream);
        if (!st) st = syldet_recordings_output_levels_device(b.r, b.ran ? (const float *)d.d_out.p : nullptr, 0, levels.buffer, b.lv_P, (float *)d.d_lv_out.p, n_readings, b.stream);
        if (!st && (hipMemcpyAsync(b.lv_in.data(), d.d_lv_in.p, b.lv_in.size() * sizeof(double), hipMemcpyDeviceToHost, b.stream) != hipSuccess ||
                    hipMemcpyAsync(b.lv_out.data(), d.d_lv_out.p, b.lv_out.size() * sizeof(float), hipMemcpyDeviceToHost, b.stream) != hipSuccess)) return 2;
    }
    if (st) std::fprintf(stderr, "Unable to meter the batch: %s: %s\n", syldet_strerror(st), syldet_last_error());
    return st ? 2 : 0;
}

// Stage 4: the counts first (a scan of the flags), then the detections themselves into tables of the size they need
int batch_events(Batch &b, BatchDevice &d)
{
    const size_t K = (size_t)b.plan.K;
    const double debounce_s = b.run.debounce_s;
    int st = syldet_recordings_events_device(b.r, nullptr, (const uint8_t *)d.d_flags.p, debounce_s, nullptr, nullptr, 0, (int64_t *)d.d_cnt.p, b.stream);
    if (!st) {
        if (hipMemcpyAsync(b.cnt.data(), d.d_cnt.p, b.cnt.size() * sizeof(int64_t), hipMemcpyDeviceToHost, b.stream) != hipSuccess || hipStreamSynchronize(b.stream) != hipSuccess) return 2;
        b.cap = std::max<int64_t>(1, *std::max_element(b.cnt.begin(), b.cnt.end()));
        b.idx.resize(K * (size_t)b.cap);
        b.val.resize(K * (size_t)b.cap * (size_t)b.n_out);
        if (!d.d_idx.alloc(b.idx.size() * sizeof(int64_t)) || !d.d_val.alloc(b.val.size() * sizeof(float))) return 2;
        st = syldet_recordings_events_device(b.r, (const float *)d.d_out.p, (const uint8_t *)d.d_flags.p, debounce_s, (int64_t *)d.d_idx.p, (float *)d.d_val.p, b.cap, (int64_t *)d.d_cnt.p, b.stream);
    }
    if (st) {
        std::fprintf(stderr, "Unable to process the batch: %s: %s\n", syldet_strerror(st), syldet_last_error());
        return 2;
    }
    if (hipMemcpyAsync(b.idx.data(), d.d_idx.p, b.idx.size() * sizeof(int64_t), hipMemcpyDeviceToHost, b.stream) != hipSuccess ||
        hipMemcpyAsync(b.val.data(), d.d_val.p, b.val.size() * sizeof(float), hipMemcpyDeviceToHost, b.stream) != hipSuccess || hipStreamSynchronize(b.stream) != hipSuccess) return 2;
    return 0;
}

// Stage 5: the thresholds' tables of every recording in one launch over the outputs that are on the device already
int batch_score(Batch &b, BatchDevice &d)
{
    ScoreRun *score = b.run.score;
    if (!score || score->failed) return 0;
    const int32_t n_thr = (int32_t)score->thresholds.size();
    syldet_scorer_t *sc = nullptr;
    DevBuf d_table;
    std::vector<int64_t> table((size_t)b.plan.K * (size_t)n_thr * SYLDET_SCORE_COLUMNS);
    int rc = 0;
    b.st = syldet_scorer_create(b.h, b.r, score->thresholds.data(), n_thr, b.score_labels.data(), b.score_begin.data(), score->tolerance, b.run.debounce_s, &sc);
    if (!b.st && !d_table.alloc(table.size() * sizeof(int64_t))) rc = 2;
    if (!rc && !b.st) b.st = syldet_score_device(sc, (const float *)d.d_out.p, b.row_evals, score->output, (int64_t *)d_table.p, b.stream);
    if (!rc && b.st) {
        std::fprintf(stderr, "Unable to score the batch: %s: %s\n", syldet_strerror(b.st), syldet_last_error());
        score->failed = true;
    } else if (!rc && (hipMemcpyAsync(table.data(), d_table.p, table.size() * sizeof(int64_t), hipMemcpyDeviceToHost, b.stream) != hipSuccess || hipStreamSynchronize(b.stream) != hipSuccess)) {
        rc = 2;
    } else if (!rc) {
        for (size_t i = 0; i < table.size(); i++) score->totals[i % ((size_t)n_thr * SYLDET_SCORE_COLUMNS)] += table[i];
    }
    syldet_scorer_destroy(sc);
    return rc;
}

// The batch's rows as fp32 on the device: the rows the bank was fed, or -- a batch of 16-bit files -- loaded once more, as fp32, from
// the same upload.  st: what the library said.  false: no memory.
bool batch_rows(Batch &b, BatchDevice &d, const float *&rows, int &st)
{
    const BatchPlan &p = b.plan;
    rows = (const float *)d.d_rows.p;
    if (!(p.all16 && !p.converting)) return true;
    if (!d.d_al_rows.p) {
        std::vector<int64_t> off2(p.src_offset);
        std::vector<int32_t> step2(p.src_step);
        for (int64_t &o : off2) o *= 2;
        for (int32_t &q : step2) q *= 2;
        if (!d.d_al_rows.alloc((size_t)b.C * (size_t)b.row_samples * sizeof(float))) return false;
        st = syldet_recordings_load_pcm_device(b.r, d.d_src.p, p.total * 2, off2.data(), step2.data(), p.src_format.data(), (float *)d.d_al_rows.p, b.row_samples, b.stream);
    }
    rows = (const float *)d.d_al_rows.p;
    return true;
}

// --match: the matches of the template in every recording's columns, from the batch's fp32 rows.  false: device trouble.
bool batch_matches(Batch &b, BatchDevice &d)
{
    if (!b.run.match) return true;
    const float *rows = nullptr;
    int st = 0;
    if (!batch_rows(b, d, rows, st)) return false;
    if (st) std::fprintf(stderr, "Unable to match the template in the batch: %s: %s\n", syldet_strerror(st), syldet_last_error());
    if (st || !match_bank(*b.run.match, b.h, b.r, rows, b.row_samples, b.row_samples, b.C, b.plan.K, b.stream, b.matched)) {
        b.run.match->failed = true;
        b.matched.assign((size_t)b.plan.K, {});
    }
    return true;
}

// --train: the network trained on the batch's recordings, from the batch's fp32 rows.  A run whose files do not go through one batch
// is known before its first batch runs (process_batched) and trains nothing; train_finish refuses it.  false: no memory.
bool batch_train(Batch &b, BatchDevice &d)
{
    TrainRun *train = b.run.train;
    if (!train) return true;
    if (train->batches++ > 0 || train->several || train->outside || train->failed) return true;   // (refused: train_finish says why)
    const float *rows = nullptr;
    int st = 0;
    if (!batch_rows(b, d, rows, st)) return false;
    if (st) std::fprintf(stderr, "Unable to train on the batch: %s: %s\n", syldet_strerror(st), syldet_last_error());
    std::vector<std::pair<std::string, int>> names;
    for (const BatchFile &f : b.files)
        for (int t = 0; t < f.info.channels; t++) names.emplace_back(f.path, t);
    train->trained = !st && train_bank(*train, b.h, b.r, b.cfg, rows, b.row_samples, b.row_evals, b.C, names, b.stream);
    train->failed = !train->trained;
    return true;
}

// Stage 6, --align-dir: the windows of every recording's events, from the batch's arrays on the device (the outputs; the fp32 rows -- a
// batch of 16-bit files is loaded once more, as fp32, from the same upload --; the rows' columns), in one launch.  false: no memory.
bool batch_windows(Batch &b, BatchDevice &d)
{
    if (!b.run.align || b.st) return true;
    AlignRun &run = *b.run.align;
    const BatchPlan &p = b.plan;
    if (syldet_align_anchor(b.h, run.opt.source, &b.al.origin, &b.al.step, nullptr)) {
        std::fprintf(stderr, "Unable to align the events of the batch: %s: %s\n", syldet_strerror(SYLDET_ERR_UNSUPPORTED), syldet_last_error());
        return true;
    }
    b.al.events.clear();
    size_t k = 0;
    for (const BatchFile &f : b.files)
        for (int t = 0; t < f.info.channels; t++, k++)
            b.al.events.push_back(align_events_of(run, f.path, t, b.ran && b.cnt[k] ? b.idx.data() + k * (size_t)b.cap : nullptr, b.ran ? b.cnt[k] : 0));
    std::vector<syldet_slot_t> slots((size_t)std::max<int32_t>(p.K, 1));
    AlignSource src;
    src.st = syldet_recordings_slots(b.r, slots.data());
    AlignInput in{(const float *)d.d_rows.p, b.row_samples, b.row_samples, 0, (const float *)d.d_out.p, b.row_evals, b.C, {}, {}, b.stream};
    if (!src.st && run.opt.source != SYLDET_ALIGN_OUTPUTS && !batch_rows(b, d, in.rows, src.st)) return false;
    for (int32_t i = 0; i < p.K; i++) {
        in.samples.push_back(slots[(size_t)i].n_samples);
        in.evals.push_back(slots[(size_t)i].n_evals);
    }
    if (!align_source(run, b.h, in, d.d_al_cols, src, b.al.units)) return false;
    if (src.st) {
        std::fprintf(stderr, "Unable to align the events of the batch: %s: %s\n", syldet_strerror(src.st), syldet_last_error());
        return true;
    }
    b.al.made = align_windows(run, b.h, b.r, src, b.stream, b.al);
    return true;
}

// Stage 7: the tracks of every file of the batch, from the outputs and flags that are on the device
int batch_tracks(Batch &b, BatchDevice &d)
{
    const TrackDirs &dirs = b.run.opt.dirs;
    const TtlOpt &ttl = b.run.opt.ttl;
    const BatchPlan &p = b.plan;
    if (!dirs.any()) return 0;
    DevBuf d_sim, d_ttl, d_on_idx, d_on_cnt;
    const int64_t N = ttl.width_samples(b.cfg->sampling_rate), lat = ttl.latency_samples(b.cfg->sampling_rate);
    const size_t track_bytes = (size_t)p.dst_total * sizeof(int16_t);
    int st = b.st;
    if (!dirs.simulate.empty()) {
        if (!d_sim.alloc(track_bytes)) return 2;
        st = syldet_recordings_trace_device_s16(b.r, (const float *)d.d_out.p, b.run.opt.simulate_output, (int16_t *)d_sim.p, p.dst_total, p.dst_offset.data(), p.dst_step.data(), b.stream);
        if (!st && hipMemcpyAsync(b.sim_frames.data(), d_sim.p, track_bytes, hipMemcpyDeviceToHost, b.stream) != hipSuccess) return 2;
    }
    if (!st && !dirs.ttl.empty()) {
        if (!d_ttl.alloc(track_bytes)) return 2;
        st = syldet_recordings_trigger_device_s16(b.r, (const uint8_t *)d.d_flags.p, ttl.buffer, N, lat, (int16_t *)d_ttl.p, p.dst_total, p.dst_offset.data(), p.dst_step.data(), b.stream);
        if (!st && hipMemcpyAsync(b.ttl_frames.data(), d_ttl.p, track_bytes, hipMemcpyDeviceToHost, b.stream) != hipSuccess) return 2;
    }
    if (!st && !dirs.onsets.empty()) {
        std::vector<syldet_slot_t> slots((size_t)p.K);
        st = syldet_recordings_slots(b.r, slots.data());
        for (const syldet_slot_t &sl : slots) b.on_cap = std::max<int64_t>(b.on_cap, std::min<int64_t>(sl.n_evals, sl.n_samples / ttl.buffer + 1));
        b.on_idx.assign((size_t)p.K * (size_t)b.on_cap, 0);
        if (!d_on_idx.alloc(b.on_idx.size() * sizeof(int64_t)) || !d_on_cnt.alloc(b.on_cnt.size() * sizeof(int64_t))) return 2;
        if (!st) st = syldet_recordings_trigger_onsets_device(b.r, (const uint8_t *)d.d_flags.p, ttl.buffer, N, lat, (int64_t *)d_on_idx.p, b.on_cap, (int64_t *)d_on_cnt.p, b.stream);
        if (!st && (hipMemcpyAsync(b.on_idx.data(), d_on_idx.p, b.on_idx.size() * sizeof(int64_t), hipMemcpyDeviceToHost, b.stream) != hipSuccess ||
                    hipMemcpyAsync(b.on_cnt.data(), d_on_cnt.p, b.on_cnt.size() * sizeof(int64_t), hipMemcpyDeviceToHost, b.stream) != hipSuccess)) return 2;
    }
    if (st) {
        std::fprintf(stderr, "Unable to make the tracks of the batch: %s: %s\n", syldet_strerror(st), syldet_last_error());
        return 2;
    }
    return hipStreamSynchronize(b.stream) != hipSuccess ? 2 : 0;
}

// Stages 2 to 7 in their order on the stream.  0, or 2: device trouble.
int batch_on_device(Batch &b, BatchDevice &d)
{
    if (int rc = load_and_run(b, d)) return rc < 0 ? 0 : rc;
    if (int rc = batch_meters(b, d)) return rc;
    if (!b.ran) return !batch_windows(b, d) || !batch_matches(b, d) || !batch_train(b, d) || hipStreamSynchronize(b.stream) != hipSuccess ? 2 : 0;   // no file of the batch has an evaluation: no events (labels may still be aligned)
    if (int rc = batch_events(b, d)) return rc;
    if (int rc = batch_score(b, d)) return rc;
    if (!batch_windows(b, d) || !batch_matches(b, d) || !batch_train(b, d)) return 2;
    return batch_tracks(b, d);
}

// Stage 8: file by file, the lines process_file prints: the tracks' events interleaved buffer by buffer (main.swift:126-130); the
// file's tracks behind its lines, which a failing write must not cost (process_file's order and its messages); its windows at the
// events, with their table (process_file's files); and its level table, line for line what process_file writes.  true: all written.
bool batch_write(const Batch &b, int rc)
{
    const Options &o = b.run.opt;
    const BatchPlan &p = b.plan;
    const double rate = b.cfg->sampling_rate;
    size_t k0 = 0;
    bool written = true;
    for (size_t i = 0; i < b.files.size(); i++) {
        const BatchFile &f = b.files[i];
        const int tracks = f.info.channels;
        const int64_t n = p.lengths[k0];
        if (o.audio.size() > 1) std::printf("%s\n", f.path.c_str());  // main.swift:122-124
        std::vector<TrackEvents> events;
        for (size_t k = k0; !rc && k < k0 + (size_t)tracks; k++)
            events.push_back({b.cnt[k] ? b.idx.data() + k * (size_t)b.cap : nullptr, nullptr, b.cnt[k], b.cnt[k] ? b.val.data() + k * (size_t)b.cap * b.n_out : nullptr});
        print_events(events, b.n_out, o.chunk, rate);
        if (rc) {
            k0 += (size_t)tracks;
            continue;
        }
        const std::string ons = TrackDirs::in(o.dirs.onsets, f.path, ".tsv");
        if (!write_track(TrackDirs::in(o.dirs.simulate, f.path), rate, tracks, n, b.sim_frames.data() + p.frames_at[i])) written = false;
        if (!write_track(TrackDirs::in(o.dirs.ttl, f.path), rate, tracks, n, b.ttl_frames.data() + p.frames_at[i])) written = false;
        if (!ons.empty() && !write_onsets(ons, tracks, b.on_idx.empty() ? nullptr : b.on_idx.data() + k0 * (size_t)b.on_cap, b.on_cnt.data() + k0, b.on_cap, rate)) written = false;
        if (b.run.align && align_write_file(*b.run.align, f.path, b.al, k0, tracks, rate)) written = false;
        if (b.run.match) match_add_file(*b.run.match, f.path, b.matched, k0, tracks, (size_t)b.plan.K);
        if (!o.dirs.levels.empty()) {
            const LevelTable table{tracks, o.levels.buffer, b.lv_P, b.lv_first[k0 + 1] - b.lv_first[k0], n, b.lv_first.data() + k0, b.lv_in.data(), b.lv_out.data(), b.lv_empty.data()};
            if (!write_levels(TrackDirs::in(o.dirs.levels, f.path, ".tsv"), table, rate)) written = false;
        }
        k0 += (size_t)tracks;
    }
    return written;
}

// One batch: returns 0, 2 for device trouble (no line of the batch is printed then, but the files' names are), or 3: the lines are
// out, a track is not
int run_batch(const Run &run, std::vector<BatchFile> &files)
{
    if (files.empty()) return 0;
    const Options &o = run.opt;
    Batch b{run, files, plan_batch(files, run.cfgs[0]->sampling_rate), run.cfgs[0]};
    const BatchPlan &p = b.plan;
    try {
        if (!o.dirs.simulate.empty()) b.sim_frames.assign((size_t)p.dst_total, 0);
        if (!o.dirs.ttl.empty()) b.ttl_frames.assign((size_t)p.dst_total, 0);
        if (!o.dirs.onsets.empty()) b.on_cnt.assign((size_t)p.K, 0);
    } catch (const std::bad_alloc &) {
        std::fprintf(stderr, "Unable to process the batch: out of memory.\n");
        files.clear();
        return 2;
    }
    b.C = (int)std::max<long>((long)run.cfgs.size(), std::min<long>(o.batch.rows, p.K));
    b.cnt.assign((size_t)p.K, 0);
    b.lv_P = levels_period_buffers(o.levels, b.cfg->sampling_rate);
    b.lv_first.assign((size_t)p.K + 1, 0);
    // --score: a track without labels, or with an evaluation-less file, still counts: its labels are misses at every threshold
    if (run.score) {
        for (const BatchFile &f : files)
            for (int t = 0; t < f.info.channels; t++) {
                const std::vector<int64_t> &labels = labels_of(run.score->labels, f.path, t);
                b.score_labels.insert(b.score_labels.end(), labels.begin(), labels.end());
                b.score_begin.push_back((int64_t)b.score_labels.size());
            }
        run.score->n_labels += (int64_t)b.score_labels.size();
    }
    int rc = 0;
    {
        BatchDevice d;                                      // (freed before the stream and the bank go)
        rc = batch_on_device(b, d);
    }
    if (rc == 2 && hipPeekAtLastError() != hipSuccess) std::fprintf(stderr, "Unable to process the batch: %s\n", hipGetErrorString(hipGetLastError()));
    if (b.stream) (void)hipStreamDestroy(b.stream);
    syldet_recordings_destroy(b.r);
    syldet_destroy(b.h);
    if (rc && run.score) run.score->failed = true;          // (a table without this batch would be another archive's)
    const bool written = batch_write(b, rc);
    files.clear();
    return rc ? rc : (written ? 0 : 3);
}

// The loop over the -a files under --batch: consecutive files that can share a bank (readable, the right number of tracks, at the
// network's rate or -- under --resample sinc -- at a rate the band-limited converter takes) gather until their samples pass
// --batch-bytes; any other file ends the batch and is processed alone in its place.
int process_batched(const Run &run)
{
    const Options &o = run.opt;
    const ResampleOpt &conv = o.conv;
    const double rate = run.cfgs[0]->sampling_rate;
    int rc = 0;
    std::vector<BatchFile> files;
    size_t held = 0;
    // what --align-dir adds to a batch on the device, per sample at the file's rate: the columns (4 x bins / hop bytes), the fp32 rows
    // the samples are cut from (4 bytes), nothing for the outputs
    double align_bytes_per_sample = 0.0;
    syldet_geometry_t g;
    if (run.align && syldet_config_geometry(run.cfgs[0], &g) == SYLDET_OK)
        align_bytes_per_sample = run.align->opt.source == SYLDET_ALIGN_COLUMNS ? 4.0 + 4.0 * g.bins / g.hop : run.align->opt.source == SYLDET_ALIGN_SAMPLES ? 4.0 : 0.0;
    for (const std::string &p : o.audio) {
        BatchFile f;
        f.path = p;
        std::string err;
        const bool probed = wav::probe(p, f.info, err);
        // (syldet_sinc_taps is -1 for what the converter refuses: a ratio outside [1/16, 16], a filter too wide)
        f.convert = probed && f.info.rate != rate;
        const bool rate_ok = probed && (!f.convert || (conv.sinc && syldet_sinc_taps(f.info.rate, rate, conv.zero_crossings, conv.rolloff) >= 0));
        if (probed && rate_ok && f.info.channels > 0 && f.info.frames > 0 && (run.cfgs.size() == 1 || (size_t)f.info.channels == run.cfgs.size())) {
            f.is16 = f.info.format == 1 && f.info.bits == 16;
            err.clear();
            if (wav::read_raw(p, f.info, f.raw, err)) {
                held += f.bytes() + (size_t)((double)f.info.frames * (double)f.info.channels * align_bytes_per_sample);
                files.push_back(std::move(f));
                if ((long long)held < o.batch.bytes) continue;
                if (run.train && &p != &o.audio.back()) run.train->several = true;   // more files behind a full batch: nothing is trained
                fold_status(rc, run_batch(run, files));
                held = 0;
                continue;
            }
        }
        // another rate that does not join the bank, unreadable, no tracks, the wrong number of tracks: exactly as without --batch, in its place
        if (run.train) run.train->outside = true;          // (before the batch in front of it runs: nothing is trained)
        fold_status(rc, run_batch(run, files));
        held = 0;
        if (run.score && run.score->labels.count(p)) std::fprintf(stderr, "--score: %s does not go through the bank; its labels are left out.\n", p.c_str());
        if (o.audio.size() > 1) std::printf("%s\n", p.c_str());
        std::fflush(stdout);
        fold_status(rc, process_file(run, p, products_of(o, p)));
    }
    fold_status(rc, run_batch(run, files));
    return rc;
}

}  // namespace
