// The one-file path: one audio file through a bank of its own, stage by stage over one state.
#pragma once

#include "align.hpp"
#include "match.hpp"
#include "train.hpp"
#include "wav.hpp"

namespace {

// What every path runs with: built once, behind the checks
struct Run {
    const Options &opt;
    const std::vector<syldet_config_t *> &cfgs;
    double debounce_s;                                      // 0: none
    ScoreRun *score;                                        // null: no --score
    AlignRun *align;                                        // null: no --align-dir
    MatchRun *match;                                        // null: no --match
    TrainRun *train = nullptr;                              // null: no --train
};

// What process_file writes for one audio file besides its lines (an empty path: not that one)
// simulate: a path for the Simulator's output track (ViewControllerSimulator.swift:251-344) of every track, made on the device from
// the outputs the run left there (syldet_trace_interleaved_device_s16) and written as a 16-bit WAV of as many frames as the detector
// was fed, at the network's rate
struct Products {
    std::string simulate;
    LevelsOpt levels;
    TtlOpt ttl;
};

// ... for file p: what the options for one file name, or p's name in every *-dir given
Products products_of(const Options &o, const std::string &p)
{
    Products w{o.dirs.simulate.empty() ? o.simulate : TrackDirs::in(o.dirs.simulate, p), o.levels, o.ttl};
    if (!o.dirs.levels.empty()) w.levels.path = TrackDirs::in(o.dirs.levels, p, ".tsv");
    if (!o.dirs.ttl.empty()) w.ttl.path = TrackDirs::in(o.dirs.ttl, p);
    if (!o.dirs.onsets.empty()) w.ttl.onsets = TrackDirs::in(o.dirs.onsets, p, ".tsv");
    return w;
}

// One track's detections: the samples, and the evaluations they were made at
struct Found { std::vector<int64_t> sample, eval; };

// events: sample number of evaluation e = first_index + e*hop (TrackDetector.swift:39-43,67-68); debounce :80,:99
Found debounced(const uint8_t *flags, int64_t E, const syldet_geometry_t &g, int64_t debounce_frames)
{
    Found found;
    int64_t until = -1;
    for (int64_t e = 0; e < E; e++) {
        if (!flags[e]) continue;
        const int64_t idx = (int64_t)g.first_index + e * (int64_t)g.hop;
        if (!(until < idx)) continue;
        until = idx + debounce_frames;
        found.sample.push_back(idx);
        found.eval.push_back(e);
    }
    return found;
}

struct OneFile {
    const Run &run;
    const std::string &path;
    const Products &want;
    const syldet_config_t *cfg;
    // read and probe: the file, how it travels, its detector
    wav::Info info;
    std::vector<float> frames;
    std::vector<int16_t> frames16;
    bool pcm16 = false, raw16 = false, resample = false, mux_refused = false;
    int C = 0, n_out = 0;
    syldet_t *h = nullptr;
    syldet_geometry_t g;
    hipStream_t stream = nullptr;
    // upload: frames of the file, samples the detector is fed (S, rows res_stride apart when converted), evaluations
    int64_t n = 0, S = 0, res_stride = 0, E = 0, fed = 0;
    // what comes back
    std::vector<float> out;
    std::vector<uint8_t> flags;
    std::vector<Found> found;                               // [C]
    std::vector<int16_t> track;
    std::vector<double> lv_in;                              // [C][M] mean squares
    std::vector<float> lv_out;                              // [C][M]
    std::vector<uint8_t> lv_empty;                          // [C][M] the reading holds no evaluation
    std::vector<int64_t> lv_first;                          // [C]
    int64_t lv_P = 1, lv_M = 0;
    std::vector<int16_t> ttl_track;                         // [S][C] or (--ttl-mux) [S][2 C]
    std::vector<int64_t> ttl_idx, ttl_cnt;                  // [C][ttl_cap], [C]
    int64_t ttl_cap = 1;
    Aligned al;                                             // --align-dir: every track's events, their windows
    std::vector<std::vector<int64_t>> matched;              // --match: every track's matches
};

// ... and what it holds on the device while it runs
struct FileDevice {
    DevBuf d_inter, d_planar, d_res, d_out, d_flags, d_track, d_lv_in, d_lv_out, d_ttl, d_ttl_idx, d_ttl_cnt, d_rows, d_al_rows, d_al_cols;
};

// Stage 1: the file's frames and the bank for its tracks.  0, 1: the file is skipped, 2: no detector.
int read_and_probe(OneFile &f)
{
    const Run &run = f.run;
    std::string err;
    // 16-bit PCM at the network's rate goes to the device as stored (syldet_run_interleaved_device_s16: the fp32 call's results
    // on x / 32768, half the bytes); any other file is decoded to fp32 here
    const bool file16 = wav::probe(f.path, f.info, err) && f.info.format == 1 && f.info.bits == 16;
    f.pcm16 = file16 && f.info.rate == f.cfg->sampling_rate;
    // ... and so does 16-bit PCM at another rate on its way to the band-limited converter, which reads int16 rows itself
    f.raw16 = f.pcm16 || (file16 && run.opt.conv.sinc);
    err.clear();
    if (f.raw16 ? !wav::read_s16(f.path, f.info, f.frames16, err) : !wav::read(f.path, f.info, f.frames, err)) {
        std::fprintf(stderr, "Unable to read %s: %s\n", f.path.c_str(), err.c_str());
        return 1;
    }
    const int C = f.C = f.info.channels;
    if (C <= 0 || f.info.frames <= 0) {
        std::fprintf(stderr, "No audio tracks found in %s.\n", f.path.c_str());
        return 1;
    }
    // (like a track that cannot be written, this does not cost the detection lines)
    f.mux_refused = f.want.ttl.mux && !f.pcm16;
    if (f.mux_refused) std::fprintf(stderr, "Unable to write %s: --ttl-mux takes 16-bit PCM at the network's sampling rate (%s).\n", f.want.ttl.path.c_str(), f.path.c_str());
    if (run.cfgs.size() > 1 && (size_t)C != run.cfgs.size()) {
        std::fprintf(stderr, "Unable to process %s: it has %d track(s), but %zu networks were given (one per track).\n", f.path.c_str(), C, run.cfgs.size());
        return 1;
    }
    std::vector<int32_t> track_net((size_t)C);
    for (int t = 0; t < C; t++) track_net[(size_t)t] = t;
    if (int st = run.cfgs.size() > 1 ? syldet_create_mixed(run.cfgs.data(), (int32_t)run.cfgs.size(), track_net.data(), C, run.opt.device, SYLDET_ENGINE_AUTO, &f.h)
                                     : syldet_create(f.cfg, C, run.opt.device, SYLDET_ENGINE_AUTO, &f.h)) {
        std::fprintf(stderr, "Unable to create the detector: %s: %s\n", syldet_strerror(st), syldet_last_error());
        return 2;
    }
    syldet_get_geometry(f.h, &f.g);
    f.n_out = f.g.outputs;
    f.resample = f.info.rate != f.cfg->sampling_rate;
    f.found.assign((size_t)C, Found());
    return 0;
}

// Stage 2: the frames to the device, and to the network's rate when the file's differs
bool upload(OneFile &f, FileDevice &d)
{
    const ResampleOpt &conv = f.run.opt.conv;
    const int C = f.C;
    if (hipSetDevice(f.run.opt.device) != hipSuccess || hipStreamCreate(&f.stream) != hipSuccess) return false;
    const int64_t n = f.n = f.info.frames;
    const size_t in_bytes = (size_t)n * C * (f.raw16 ? sizeof(int16_t) : sizeof(float));
    if (!d.d_inter.alloc(in_bytes)) return false;
    if (hipMemcpyAsync(d.d_inter.p, f.raw16 ? (const void *)f.frames16.data() : (const void *)f.frames.data(), in_bytes, hipMemcpyHostToDevice, f.stream) != hipSuccess) return false;
    f.S = n;
    if (!f.resample) return true;
    // The reference's tool has AVFoundation deliver every track at the network's rate (SyllableDetector.swift:19-23,
    // TrackDetector.swift:35); here: linear interpolation of the whole decoded file with fp64 positions
    // (syldet_convert_rate_device; ResamplerLinear is the live path's streaming object, not a file converter) or, with
    // --resample sinc, the band-limited converter -- on the int16 rows of a 16-bit file, which never become fp32 input
    const double from = f.info.rate, to = f.cfg->sampling_rate;
    const int64_t stride = f.res_stride = syldet_convert_rate_count(n, from, to);
    if (!d.d_planar.alloc((size_t)C * n * (f.raw16 ? sizeof(int16_t) : sizeof(float))) || !d.d_res.alloc((size_t)C * (stride > 0 ? stride : 1) * sizeof(float))) return false;
    int st = 0;
    if (f.raw16) {
        st = syldet_deinterleave_device_s16((const int16_t *)d.d_inter.p, n, C, C, (int16_t *)d.d_planar.p, n, f.stream);
        if (!st) st = syldet_convert_rate_sinc_device_s16((const int16_t *)d.d_planar.p, n, n, C, from, to, conv.zero_crossings, conv.beta, conv.rolloff, (float *)d.d_res.p, stride, &f.S, f.stream);
    } else {
        st = syldet_deinterleave_device((const float *)d.d_inter.p, n, C, 0, C, (float *)d.d_planar.p, n, f.stream);
        if (!st && conv.sinc) st = syldet_convert_rate_sinc_device((const float *)d.d_planar.p, n, n, C, from, to, conv.zero_crossings, conv.beta, conv.rolloff, (float *)d.d_res.p, stride, &f.S, f.stream);
        else if (!st) st = syldet_convert_rate_device((const float *)d.d_planar.p, n, n, C, from, to, (float *)d.d_res.p, stride, &f.S, f.stream);
    }
    if (st) std::fprintf(stderr, "Unable to process %s: %s: %s\n", f.path.c_str(), syldet_strerror(st), syldet_last_error());
    return st == 0;
}

// Stage 3: the run, which leaves the outputs and the flags on the device
bool run_detector(OneFile &f, FileDevice &d)
{
    if (!d.d_out.alloc((size_t)f.C * f.E * f.n_out * sizeof(float)) || !d.d_flags.alloc((size_t)f.C * f.E)) return false;
    int st = 0;
    if (f.pcm16) st = syldet_run_interleaved_device_s16(f.h, (const int16_t *)d.d_inter.p, f.n, f.C, (float *)d.d_out.p, (uint8_t *)d.d_flags.p, f.stream);
    else if (!f.resample) st = syldet_run_interleaved_device(f.h, (const float *)d.d_inter.p, f.n, f.C, (float *)d.d_out.p, (uint8_t *)d.d_flags.p, f.stream);
    else st = syldet_run_device(f.h, (const float *)d.d_res.p, f.S, f.res_stride, (float *)d.d_out.p, (uint8_t *)d.d_flags.p, f.stream);
    if (st) std::fprintf(stderr, "Unable to process %s: %s: %s\n", f.path.c_str(), syldet_strerror(st), syldet_last_error());
    return st == 0;
}

// Stage 4, the products.  The meters: the input readings of the samples the detector is fed (queued behind the copy; a recording
// shorter than one evaluation has them too), the output readings behind the run
bool meters(OneFile &f, FileDevice &d, bool outputs_too)
{
    const LevelsOpt &levels = f.want.levels;
    if (levels.path.empty() || f.S <= 0) return true;
    f.lv_P = levels_period_buffers(levels, f.cfg->sampling_rate);
    f.lv_M = syldet_levels_count(f.S, levels.buffer, f.lv_P);
    const size_t cells = (size_t)f.C * (size_t)f.lv_M;
    int st = 0;
    if (!outputs_too) {
        f.lv_in.resize(cells);
        if (!d.d_lv_in.alloc(cells * sizeof(double))) return false;
        if (f.pcm16) st = syldet_levels_interleaved_device_s16(f.h, (const int16_t *)d.d_inter.p, f.n, f.C, levels.buffer, f.lv_P, (double *)d.d_lv_in.p, f.stream);
        else if (!f.resample) st = syldet_levels_interleaved_device(f.h, (const float *)d.d_inter.p, f.n, f.C, levels.buffer, f.lv_P, (double *)d.d_lv_in.p, f.stream);
        else st = syldet_levels_device(f.h, (const float *)d.d_res.p, f.S, f.res_stride, levels.buffer, f.lv_P, (double *)d.d_lv_in.p, f.stream);
        if (!st && hipMemcpyAsync(f.lv_in.data(), d.d_lv_in.p, cells * sizeof(double), hipMemcpyDeviceToHost, f.stream) != hipSuccess) return false;
    } else {
        f.lv_out.resize(cells);
        if (!d.d_lv_out.alloc(cells * sizeof(float))) return false;
        st = syldet_output_levels_device(f.h, (const float *)d.d_out.p, f.E, 0, f.S, levels.buffer, f.lv_P, (float *)d.d_lv_out.p, f.stream);
        if (!st && hipMemcpyAsync(f.lv_out.data(), d.d_lv_out.p, cells * sizeof(float), hipMemcpyDeviceToHost, f.stream) != hipSuccess) return false;
    }
    if (st) std::fprintf(stderr, "Unable to meter %s: %s: %s\n", f.path.c_str(), syldet_strerror(st), syldet_last_error());
    return st == 0;
}

// ... the trigger tracks and their rising edges from the flags the run left on the device (no evaluation: no flag, zeros)
bool triggers(OneFile &f, FileDevice &d)
{
    const TtlOpt &ttl = f.want.ttl;
    const int C = f.C;
    const int64_t S = f.S;
    if (!ttl.any() || S <= 0) return true;
    const int64_t N = ttl.width_samples(f.cfg->sampling_rate), lat = ttl.latency_samples(f.cfg->sampling_rate), nE = f.E > 0 ? f.E : 0;
    int st = 0;
    if (!d.d_flags.p && !d.d_flags.alloc(1)) return false;
    if (!ttl.path.empty() && !f.mux_refused) {
        f.ttl_track.resize((size_t)S * C * (ttl.mux ? 2 : 1));
        if (!d.d_ttl.alloc(f.ttl_track.size() * sizeof(int16_t))) return false;
        if (ttl.mux) {
            // the recording as planar int16 rows, the layout syldet_run_device_s16 takes: from the frames already on the device
            if (!d.d_rows.alloc((size_t)C * S * sizeof(int16_t))) return false;
            st = syldet_deinterleave_device_s16((const int16_t *)d.d_inter.p, S, C, C, (int16_t *)d.d_rows.p, S, f.stream);
            if (!st) st = syldet_trigger_mux_device_s16(f.h, (const uint8_t *)d.d_flags.p, nE, ttl.buffer, N, lat, (const int16_t *)d.d_rows.p, S, (int16_t *)d.d_ttl.p, S, f.stream);
        } else {
            st = syldet_trigger_interleaved_device_s16(f.h, (const uint8_t *)d.d_flags.p, nE, ttl.buffer, N, lat, (int16_t *)d.d_ttl.p, S, f.stream);
        }
        if (!st && hipMemcpyAsync(f.ttl_track.data(), d.d_ttl.p, f.ttl_track.size() * sizeof(int16_t), hipMemcpyDeviceToHost, f.stream) != hipSuccess) return false;
    }
    if (!st && !ttl.onsets.empty()) {
        f.ttl_cap = std::max<int64_t>(1, std::min<int64_t>(nE, S / ttl.buffer + 1));
        f.ttl_idx.assign((size_t)C * (size_t)f.ttl_cap, 0);
        f.ttl_cnt.assign((size_t)C, 0);
        if (!d.d_ttl_idx.alloc(f.ttl_idx.size() * sizeof(int64_t)) || !d.d_ttl_cnt.alloc(f.ttl_cnt.size() * sizeof(int64_t))) return false;
        st = syldet_trigger_onsets_device(f.h, (const uint8_t *)d.d_flags.p, nE, ttl.buffer, N, lat, S, (int64_t *)d.d_ttl_idx.p, f.ttl_cap, (int64_t *)d.d_ttl_cnt.p, f.stream);
        if (!st && (hipMemcpyAsync(f.ttl_idx.data(), d.d_ttl_idx.p, f.ttl_idx.size() * sizeof(int64_t), hipMemcpyDeviceToHost, f.stream) != hipSuccess ||
                    hipMemcpyAsync(f.ttl_cnt.data(), d.d_ttl_cnt.p, f.ttl_cnt.size() * sizeof(int64_t), hipMemcpyDeviceToHost, f.stream) != hipSuccess)) return false;
    }
    if (st) std::fprintf(stderr, "Unable to make the trigger track of %s: %s: %s\n", f.path.c_str(), syldet_strerror(st), syldet_last_error());
    return st == 0;
}

// ... the Simulator's track from the outputs
bool trace(OneFile &f, FileDevice &d)
{
    if (f.want.simulate.empty()) return true;
    f.track.resize((size_t)f.S * f.C);
    if (!d.d_track.alloc(f.track.size() * sizeof(int16_t))) return false;
    if (int st = syldet_trace_interleaved_device_s16(f.h, (const float *)d.d_out.p, f.E, f.run.opt.simulate_output, (int16_t *)d.d_track.p, f.S, f.stream)) {
        std::fprintf(stderr, "Unable to simulate %s: %s: %s\n", f.path.c_str(), syldet_strerror(st), syldet_last_error());
        return false;
    }
    return hipMemcpyAsync(f.track.data(), d.d_track.p, f.track.size() * sizeof(int16_t), hipMemcpyDeviceToHost, f.stream) == hipSuccess;
}

// The file's tracks as fp32 rows on the device, what the detector was fed: the converter's rows, or (once) the decoded frames
// (16-bit PCM: x * 2^-15, exact).  false: no memory.
bool file_rows(OneFile &f, FileDevice &d, const float *&rows, int64_t &stride)
{
    const int C = f.C;
    const int64_t S = f.S;
    if (f.resample) {
        rows = (const float *)d.d_res.p;
        stride = f.res_stride;
        return true;
    }
    stride = S;
    if (!d.d_al_rows.p) {
        std::vector<float> planar((size_t)C * (size_t)S);
        for (int64_t i = 0; i < S; i++)
            for (int c = 0; c < C; c++)
                planar[(size_t)c * (size_t)S + (size_t)i] = f.raw16 ? (float)f.frames16[(size_t)i * C + c] * (1.0f / 32768.0f) : f.frames[(size_t)i * C + c];
        if (!d.d_al_rows.alloc(planar.size() * sizeof(float)) || hipMemcpy(d.d_al_rows.p, planar.data(), planar.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return false;
    }
    rows = (const float *)d.d_al_rows.p;
    return true;
}

// ... the matches of the template in every track's columns (--match), from the fp32 rows the detector was fed
void matches(OneFile &f, FileDevice &d)
{
    if (!f.run.match) return;
    const float *rows = nullptr;
    int64_t stride = f.S;
    f.matched.assign((size_t)f.C, {});
    if (!file_rows(f, d, rows, stride) || !match_bank(*f.run.match, f.h, nullptr, rows, f.S, stride, f.C, f.C, f.stream, f.matched)) {
        std::fprintf(stderr, "Unable to match the template in %s.\n", f.path.c_str());
        f.run.match->failed = true;
    }
}

// ... the windows of every track's events (--align-dir), from arrays on the device: the outputs the run left, the fp32 rows the
// detector was fed, or their columns (syldet_spectrogram_device).  Behind the download of the flags: the detections are made
// from them.  (Windows that cannot be made do not cost the lines: write_files reports them.)
void windows(OneFile &f, FileDevice &d)
{
    if (!f.run.align) return;
    AlignRun &run = *f.run.align;
    const int C = f.C;
    const int64_t S = f.S;
    if (syldet_align_anchor(f.h, run.opt.source, &f.al.origin, &f.al.step, nullptr)) {
        std::fprintf(stderr, "Unable to align the events of %s: %s: %s\n", f.path.c_str(), syldet_strerror(SYLDET_ERR_UNSUPPORTED), syldet_last_error());
        return;                                             // (no files for it)
    }
    f.al.events.clear();
    for (int c = 0; c < C; c++) f.al.events.push_back(align_events_of(run, f.path, c, f.found[(size_t)c].sample.data(), (int64_t)f.found[(size_t)c].sample.size()));
    AlignInput in{nullptr, S, S, 0, (const float *)d.d_out.p, f.E > 0 ? f.E : 0, C, {}, {}, f.stream};
    if (run.opt.source != SYLDET_ALIGN_OUTPUTS && !file_rows(f, d, in.rows, in.stride)) return;
    in.samples_stride = in.stride;
    in.samples.assign((size_t)C, S);
    in.evals.assign((size_t)C, in.row_evals);
    AlignSource src;
    if (!align_source(run, f.h, in, d.d_al_cols, src, f.al.units)) return;
    if (src.st) {
        std::fprintf(stderr, "Unable to align the events of %s: %s: %s\n", f.path.c_str(), syldet_strerror(src.st), syldet_last_error());
        return;
    }
    f.al.made = align_windows(run, f.h, nullptr, src, f.stream, f.al);
}

// Stage 5: the outputs and the flags come back, and every track's detections are made of them
bool download(OneFile &f, FileDevice &d)
{
    const int64_t debounce_frames = (int64_t)(f.run.debounce_s * f.cfg->sampling_rate);   // Int(newValue * samplingRate), TrackDetector.swift:24
    f.out.resize((size_t)f.C * f.E * f.n_out);
    f.flags.resize((size_t)f.C * f.E);
    if (hipMemcpyAsync(f.out.data(), d.d_out.p, f.out.size() * sizeof(float), hipMemcpyDeviceToHost, f.stream) != hipSuccess ||
        hipMemcpyAsync(f.flags.data(), d.d_flags.p, f.flags.size(), hipMemcpyDeviceToHost, f.stream) != hipSuccess ||
        hipStreamSynchronize(f.stream) != hipSuccess) return false;
    for (int c = 0; c < f.C; c++) f.found[(size_t)c] = debounced(f.flags.data() + (size_t)c * f.E, f.E, f.g, debounce_frames);
    return true;
}

// Stages 2 to 5 in their order on the stream.  0, or 2: device trouble.
int on_device(OneFile &f, FileDevice &d)
{
    if (!upload(f, d)) return 2;
    f.E = syldet_count_evals(f.h, f.S);
    f.fed = f.S;
    if (f.E <= 0 && !f.want.simulate.empty()) f.track.assign((size_t)f.S * f.C, 0);   // shorter than one evaluation: a track of zeros
    if (!meters(f, d, false)) return 2;
    if (f.E <= 0) {                                         // shorter than one evaluation: no events
        if (!triggers(f, d)) return 2;
        if ((!f.want.levels.path.empty() || f.want.ttl.any()) && hipStreamSynchronize(f.stream) != hipSuccess) return 2;
        windows(f, d);
        matches(f, d);
        return 0;
    }
    if (!run_detector(f, d) || !trace(f, d) || !meters(f, d, true) || !triggers(f, d) || !download(f, d)) return 2;
    windows(f, d);
    matches(f, d);
    return 0;
}

// a 16-bit track file (an empty path: none).  false: it could not be written.
bool write_track(const std::string &path, double rate, int tracks, int64_t n, const int16_t *frames)
{
    std::string werr;
    if (path.empty() || wav::write_s16(path, rate, tracks, n, frames, werr)) return true;
    std::fprintf(stderr, "Unable to write %s: %s\n", path.c_str(), werr.c_str());
    return false;
}

// Stage 7: the files are written behind the detection lines, which a failing write must not cost: 3 = the lines are out, a file is
// not.  The track; the meters' readings; the trigger tracks and their rising edges; the windows at the events, with their table
// (and the events into the stacks).
int write_files(OneFile &f)
{
    const double rate = f.cfg->sampling_rate;
    const TtlOpt &ttl = f.want.ttl;
    int a = 0, b = 0, c = f.mux_refused ? 3 : 0;
    if (!write_track(f.want.simulate, rate, f.C, f.fed, f.track.data())) a = 3;
    const LevelTable table{f.C, f.want.levels.buffer, f.lv_P, f.lv_M, f.fed, f.lv_first.data(), f.lv_in.data(), f.lv_out.data(), f.lv_empty.data()};
    if (!f.want.levels.path.empty() && !write_levels(f.want.levels.path, table, rate)) b = 3;
    if (!f.mux_refused && !write_track(ttl.path, rate, ttl.mux ? 2 * f.C : f.C, f.fed, f.ttl_track.data())) c = 3;
    if (!ttl.onsets.empty() && !write_onsets(ttl.onsets, f.ttl_cnt.empty() ? 0 : f.C, f.ttl_idx.data(), f.ttl_cnt.data(), f.ttl_cap, rate)) c = 3;
    const int w = f.run.align ? align_write_file(*f.run.align, f.path, f.al, 0, f.C, rate) : 0;
    if (f.run.match) match_add_file(*f.run.match, f.path, f.matched, 0, f.C, (size_t)f.C);
    return a ? a : (b ? b : (c ? c : w));
}

// cfgs: one network for every track, or (k > 1) network t for track t of a file of exactly k tracks, through one mixed bank
// (syldet_create_mixed): the networks share the evaluation clock, so the events are found and printed as for one
int process_file(const Run &run, const std::string &path, const Products &want)
{
    OneFile f{run, path, want, run.cfgs[0]};
    if (int r = read_and_probe(f)) return r;
    int rc = 0;
    {
        FileDevice d;                                       // (freed before the stream and the detector go)
        rc = on_device(f, d);
    }
    if (rc == 2 && hipPeekAtLastError() != hipSuccess) std::fprintf(stderr, "Unable to process %s: %s\n", path.c_str(), hipGetErrorString(hipGetLastError()));
    if (f.stream) (void)hipStreamDestroy(f.stream);
    if (!rc && !want.levels.path.empty()) {
        f.lv_empty.assign((size_t)f.C * (size_t)f.lv_M, 1);
        for (int64_t m = 0; m < f.lv_M; m++) {
            int64_t first = 0, count = 0;
            if (syldet_levels_eval_range(f.h, f.fed, f.E > 0 ? f.E : 0, want.levels.buffer, f.lv_P, m, &first, &count) != SYLDET_OK) continue;
            for (int c = 0; c < f.C; c++) f.lv_empty[(size_t)c * (size_t)f.lv_M + (size_t)m] = count == 0;
        }
        for (int c = 0; c < f.C; c++) f.lv_first.push_back(c * f.lv_M);
    }
    syldet_destroy(f.h);
    if (rc) return rc;
    if (f.E <= 0) return write_files(f);
    // Stage 6: the lines
    std::vector<TrackEvents> tracks;
    for (int c = 0; c < f.C; c++) {
        const Found &found = f.found[(size_t)c];
        tracks.push_back({found.sample.data(), found.eval.data(), (int64_t)found.sample.size(), f.out.data() + (size_t)c * f.E * f.n_out});
    }
    print_events(tracks, f.n_out, run.opt.chunk, f.cfg->sampling_rate);
    return write_files(f);
}

}  // namespace
