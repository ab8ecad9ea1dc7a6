// --match: the template and what a run gathers (see MatchOpt), the matches of one bank's detectors, and the file written at the end.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>

#include "align.hpp"

namespace {

struct MatchRun {
    MatchOpt opt;
    std::vector<float> templ;                              // [n][bins]
    int n = 0, bins = 0, anchor = -1, separation = 0;      // the separation in frames
    float threshold = 0.0f;
    std::string lines;                                      // file<TAB>track<TAB>sample, in command-line order, then track, then sample
    bool failed = false;
};

// A NumPy file (format 1.0 or 2.0) of a little-endian float32 or float64 C-order array of two dimensions -> float32 values.
bool read_npy(const std::string &path, std::vector<float> &values, int64_t shape[2], std::string &err)
{
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { err = "unable to open " + path; return false; }
    std::string bytes;
    char buf[65536];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) bytes.append(buf, k);
    std::fclose(f);
    const auto bad = [&](const char *why) { err = path + ": " + why; return false; };
    if (bytes.size() < 12 || std::memcmp(bytes.data(), "\x93NUMPY", 6) != 0) return bad("not a NumPy file");
    const unsigned major = (unsigned char)bytes[6];
    size_t hlen = 0, at = 0;
    if (major == 1) { hlen = (unsigned char)bytes[8] | ((size_t)(unsigned char)bytes[9] << 8); at = 10; }
    else if (major == 2) { for (int k = 0; k < 4; k++) hlen |= (size_t)(unsigned char)bytes[8 + k] << (8 * k); at = 12; }
    else return bad("a NumPy format other than 1.0 and 2.0");
    if (hlen > bytes.size() - at) return bad("a truncated header");
    const std::string head = bytes.substr(at, hlen);
    const bool f4 = head.find("'<f4'") != std::string::npos, f8 = head.find("'<f8'") != std::string::npos;
    if (!f4 && !f8) return bad("not little-endian float32 or float64");
    if (head.find("'fortran_order': False") == std::string::npos) return bad("not in C order");
    const size_t sh = head.find("'shape': (");
    if (sh == std::string::npos) return bad("no shape");
    const char *p = head.c_str() + sh + 10;
    char *end = nullptr;
    int dims = 0;
    while (*p && *p != ')') {
        const long long v = std::strtoll(p, &end, 10);
        if (end == p || v < 0 || dims == 2) return bad("not an array [frames][bins]");
        shape[dims++] = v;
        p = end;
        while (*p == ',' || *p == ' ') p++;
    }
    if (dims != 2 || shape[0] < 1 || shape[1] < 1 || shape[0] > SYLDET_MATCH_MAX_TEMPLATE || shape[1] > SYLDET_MATCH_MAX_TEMPLATE ||
        shape[0] * shape[1] > SYLDET_MATCH_MAX_TEMPLATE)
        return bad("not an array [frames][bins] of 1 to 32768 values");
    const size_t count = (size_t)(shape[0] * shape[1]), el = f4 ? 4 : 8;
    if (bytes.size() - at - hlen < count * el) return bad("fewer values than the shape says");
    values.resize(count);
    const char *data = bytes.data() + at + hlen;
    for (size_t k = 0; k < count; k++) {
        if (f4) std::memcpy(&values[k], data + 4 * k, 4);
        else { double v; std::memcpy(&v, data + 8 * k, 8); values[k] = (float)v; }
    }
    return true;
}

// The template, and the options in the network's units.  0, or the usage error.
int match_begin(MatchRun &run, const MatchOpt &opt, const std::vector<syldet_config_t *> &cfgs)
{
    run.opt = opt;
    if (cfgs.size() > 1) return fail("--match takes one network (-n): the columns of several are ragged.");
    syldet_geometry_t g;
    if (const int st = syldet_config_geometry(cfgs[0], &g)) return fail(std::string("Unable to use the network configuration: ") + syldet_strerror(st) + ": " + syldet_last_error());
    std::string err;
    int64_t shape[2] = {0, 0};
    if (!read_npy(opt.path, run.templ, shape, err)) return fail("--match: " + err + ".");
    run.n = (int)shape[0];
    run.bins = (int)shape[1];
    if (run.bins != g.bins) return fail("--match: the template has " + std::to_string(run.bins) + " bins, the network's columns " + std::to_string(g.bins) + ".");
    std::vector<float> t_hat(run.templ.size());
    if (syldet_match_normalize_host(run.templ.data(), run.n, run.bins, t_hat.data())) return fail(std::string("--match: ") + syldet_last_error() + ".");
    if (opt.anchor >= run.n) return fail("--match-anchor takes a frame of the template, 0 to " + std::to_string(run.n - 1) + ".");
    run.anchor = opt.anchor < 0 ? run.n - 1 : (int)opt.anchor;
    run.threshold = (float)opt.threshold;
    // the separation in frames: the template's own length unless given
    const double frames = opt.separation < 0.0 ? (double)run.n : opt.separation * cfgs[0]->sampling_rate / (double)g.hop;
    if (!(frames <= (double)SYLDET_MATCH_MAX_SEPARATION)) return fail("--match-separation may be " + std::to_string(SYLDET_MATCH_MAX_SEPARATION) + " frames at most.");
    run.separation = (int)frames;
    return 0;
}

// The matches of one bank's detectors -- a batch's recordings (r), or a file's tracks (r NULL) -- from the fp32 rows the bank was fed:
// the rows' columns, the scores, the peaks (twice where the first table is too small), and back.  false: the device's or the library's refusal.
bool match_bank(MatchRun &run, syldet_t *h, syldet_recordings_t *r, const float *rows, int64_t row_samples, int64_t stride, int C, int D, hipStream_t stream,
                std::vector<std::vector<int64_t>> &events)
{
    events.assign((size_t)D, {});
    const int64_t J = std::max<int64_t>(0, syldet_count_frames(h, row_samples));
    if (J <= 0 || D <= 0) return true;
    syldet_matcher_t *m = nullptr;
    int st = syldet_matcher_create(h, r, run.templ.data(), run.n, run.bins, run.anchor, &m);
    DevBuf d_cols, d_scores, d_events, d_counts;
    bool ok = true;
    std::vector<int64_t> counts((size_t)D, 0), table;
    int64_t cap = 1024;
    if (!st) {
        ok = d_cols.alloc((size_t)C * (size_t)J * (size_t)run.bins * sizeof(float)) && d_scores.alloc((size_t)C * (size_t)J * sizeof(float)) &&
             d_counts.alloc((size_t)D * sizeof(int64_t));
        if (ok) st = syldet_spectrogram_device(h, rows, row_samples, stride, (float *)d_cols.p, stream);
        if (ok && !st) st = syldet_match_scores_device(m, (const float *)d_cols.p, J, 0, (float *)d_scores.p, stream);
        for (int pass = 0; ok && !st && pass < 2; pass++) {
            DevBuf d_table;
            ok = d_table.alloc((size_t)D * (size_t)cap * sizeof(int64_t));
            if (ok) st = syldet_match_peaks_device(m, (const float *)d_scores.p, J, run.threshold, run.separation, (int64_t *)d_table.p, cap, (int64_t *)d_counts.p, nullptr, stream);
            table.assign((size_t)D * (size_t)cap, 0);
            if (ok && !st)
                ok = hipMemcpyAsync(counts.data(), d_counts.p, counts.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream) == hipSuccess &&
                     hipMemcpyAsync(table.data(), d_table.p, table.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream) == hipSuccess &&
                     hipStreamSynchronize(stream) == hipSuccess;
            const int64_t most = *std::max_element(counts.begin(), counts.end());
            if (most <= cap) break;
            cap = most;                                     // a table too small: once more with the largest count
        }
    }
    syldet_matcher_destroy(m);
    if (st) std::fprintf(stderr, "Unable to match the template: %s: %s\n", syldet_strerror(st), syldet_last_error());
    if (!ok || st) return false;
    for (int d = 0; d < D; d++) events[(size_t)d].assign(table.begin() + (size_t)d * (size_t)cap, table.begin() + (size_t)d * (size_t)cap + (size_t)std::min(counts[(size_t)d], cap));
    return true;
}

// one file's lines: its tracks are the bank's detectors k0 .. k0 + tracks - 1
void match_add_file(MatchRun &run, const std::string &path, const std::vector<std::vector<int64_t>> &events, size_t k0, int tracks)
{
    for (size_t t = 0; t < (size_t)tracks && k0 + t < events.size(); t++)
        for (const int64_t s : events[k0 + t]) run.lines += path + "\t" + std::to_string(t) + "\t" + std::to_string(s) + "\n";
}

// the file, behind the last audio file
bool match_finish(const MatchRun &run)
{
    FILE *f = std::fopen(run.opt.out_path.c_str(), "wb");
    bool ok = f != nullptr && std::fwrite(run.lines.data(), 1, run.lines.size(), f) == run.lines.size();
    if (f && std::fclose(f) != 0) ok = false;
    if (!ok) std::fprintf(stderr, "Unable to write %s.\n", run.opt.out_path.c_str());
    return ok && !run.failed;
}

}  // namespace
