// --match: the templates and what a run gathers (see MatchOpt), the matches of one bank's detectors, and the files written at the end.
// The i-th --match is class i of one bank of templates (syldet_matcher_bank_*): one scores call and one peaks call a bank of
// detectors, whatever the number of classes and exemplars.  Files that all share their frame count make the uniform bank; with
// --match-ragged files of different frame counts make a ragged one (syldet_matcher_bank_create_ragged), whose planes are indexed by
// the anchor frame.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <functional>

#include "align.hpp"

namespace {

struct MatchRun {
    MatchOpt opt;
    std::vector<float> templ;                              // [K][n][bins], class by class (ragged: each [n_k][bins], one after another)
    std::vector<int32_t> tclass;                           // [K]
    std::vector<int32_t> tn, ta;                           // [K] every template's frames and anchor frame
    std::vector<int32_t> class_n;                          // [C] the frames of a class's file
    std::vector<float> thresholds;                         // [C]
    std::vector<int32_t> separations;                      // [C] in frames
    bool ragged = false;                                   // the files differ in their frame counts
    int K = 0, C = 0, n = 0, bins = 0, anchor = -1;        // n, anchor: the uniform bank's
    std::vector<std::string> lines;                        // [C] file<TAB>track<TAB>sample, in command-line order, then track, then sample
    bool failed = false;
};

// A NumPy file (format 1.0 or 2.0) of a little-endian float32 or float64 C-order array [frames][bins] or [exemplars][frames][bins] ->
// float32 values and shape = {exemplars (1 for two dimensions), frames, bins}.
bool read_npy(const std::string &path, std::vector<float> &values, int64_t shape[3], std::string &err)
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
        if (end == p || v < 0 || dims == 3) return bad("not an array [frames][bins]");
        shape[dims++] = v;
        p = end;
        while (*p == ',' || *p == ' ') p++;
    }
    if (dims == 2) {
        shape[2] = shape[1];
        shape[1] = shape[0];
        shape[0] = 1;
    }
    if (dims < 2 || shape[1] < 1 || shape[2] < 1 || shape[1] > SYLDET_MATCH_MAX_TEMPLATE || shape[2] > SYLDET_MATCH_MAX_TEMPLATE ||
        shape[1] * shape[2] > SYLDET_MATCH_MAX_TEMPLATE)
        return bad("not an array [frames][bins] of 1 to 32768 values");
    if (shape[0] < 1 || shape[0] > SYLDET_MATCH_MAX_TEMPLATES) return bad("not 1 to 64 exemplars [exemplars][frames][bins]");
    const size_t count = (size_t)(shape[0] * shape[1] * shape[2]), el = f4 ? 4 : 8;
    if (bytes.size() - at - hlen < count * el) return bad("fewer values than the shape says");
    values.resize(count);
    const char *data = bytes.data() + at + hlen;
    for (size_t k = 0; k < count; k++) {
        if (f4) std::memcpy(&values[k], data + 4 * k, 4);
        else { double v; std::memcpy(&v, data + 8 * k, 8); values[k] = (float)v; }
    }
    return true;
}

// The templates, and the options in the network's units.  0, or the usage error.
int match_begin(MatchRun &run, const MatchOpt &opt, const std::vector<syldet_config_t *> &cfgs)
{
    run.opt = opt;
    if (cfgs.size() > 1) return fail("--match takes one network (-n): the columns of several are ragged.");
    syldet_geometry_t g;
    if (const int st = syldet_config_geometry(cfgs[0], &g)) return fail(std::string("Unable to use the network configuration: ") + syldet_strerror(st) + ": " + syldet_last_error());
    run.C = (int)opt.paths.size();
    run.lines.assign((size_t)run.C, std::string());
    for (int c = 0; c < run.C; c++) {
        std::string err;
        std::vector<float> values;
        int64_t shape[3] = {0, 0, 0};
        if (!read_npy(opt.paths[(size_t)c], values, shape, err)) return fail("--match: " + err + ".");
        if (c == 0) {
            run.n = (int)shape[1];
            run.bins = (int)shape[2];
            if (run.bins != g.bins) return fail("--match: the template has " + std::to_string(run.bins) + " bins, the network's columns " + std::to_string(g.bins) + ".");
        } else if (shape[2] != run.bins || (shape[1] != run.n && !opt.ragged)) {
            return fail("--match: " + opt.paths[0] + " is [" + std::to_string(run.n) + "][" + std::to_string(run.bins) + "] and " + opt.paths[(size_t)c] + " [" +
                        std::to_string(shape[1]) + "][" + std::to_string(shape[2]) + "]: the templates of one run share their frames and bins (--match-ragged: their bins).");
        }
        const int n = (int)shape[1];
        run.ragged = run.ragged || n != run.n;
        run.class_n.push_back(n);
        run.K += (int)shape[0];
        if (run.K > SYLDET_MATCH_MAX_TEMPLATES) return fail("--match takes " + std::to_string(SYLDET_MATCH_MAX_TEMPLATES) + " exemplars at most, all files together.");
        const size_t one = (size_t)n * (size_t)run.bins;
        std::vector<float> t_hat(one);
        for (int64_t k = 0; k < shape[0]; k++)
            if (syldet_match_normalize_host(values.data() + (size_t)k * one, n, run.bins, t_hat.data())) return fail(std::string("--match: ") + syldet_last_error() + ".");
        run.templ.insert(run.templ.end(), values.begin(), values.end());
        run.tclass.insert(run.tclass.end(), (size_t)shape[0], c);
        run.tn.insert(run.tn.end(), (size_t)shape[0], n);
    }
    // the anchors: each class's last frame unless given; one for all is a frame of the shortest template
    const int shortest = *std::min_element(run.class_n.begin(), run.class_n.end());
    if (opt.anchors.size() == 1 && opt.anchors[0] >= shortest)
        return fail("--match-anchor takes a frame of the template, 0 to " + std::to_string(shortest - 1) + ".");
    std::vector<int32_t> class_anchor;
    for (int c = 0; c < run.C; c++) {
        const int n = run.class_n[(size_t)c];
        const long a = opt.anchors.empty() ? n - 1 : opt.anchors[opt.anchors.size() == 1 ? 0 : (size_t)c];
        if (a >= n) return fail("--match-anchor takes a frame of the template: " + opt.paths[(size_t)c] + " has the frames 0 to " + std::to_string(n - 1) + ".");
        class_anchor.push_back((int32_t)a);
    }
    for (int k = 0; k < run.K; k++) run.ta.push_back(class_anchor[(size_t)run.tclass[(size_t)k]]);
    // (files of one length with an anchor a class are lined up at their anchors too: the ragged bank)
    run.ragged = run.ragged || std::adjacent_find(class_anchor.begin(), class_anchor.end(), std::not_equal_to<int32_t>()) != class_anchor.end();
    run.anchor = class_anchor[0];
    for (int c = 0; c < run.C; c++)
        run.thresholds.push_back((float)(opt.thresholds.empty() ? 0.77 : opt.thresholds[opt.thresholds.size() == 1 ? 0 : (size_t)c]));
    // the separations in frames: each class's own length unless given
    for (int c = 0; c < run.C; c++) {
        const double frames = opt.separations.empty() ? (double)run.class_n[(size_t)c]
                                                      : opt.separations[opt.separations.size() == 1 ? 0 : (size_t)c] * cfgs[0]->sampling_rate / (double)g.hop;
        if (!(frames <= (double)SYLDET_MATCH_MAX_SEPARATION)) return fail("--match-separation may be " + std::to_string(SYLDET_MATCH_MAX_SEPARATION) + " frames at most.");
        run.separations.push_back((int32_t)frames);
    }
    return 0;
}

// The matches of one bank's detectors -- a batch's recordings (r), or a file's tracks (r NULL) -- from the fp32 rows the bank was fed:
// the rows' columns, every class's scores in one call, every class's peaks in one call (twice where the first table is too small),
// and back: events [class * D + detector].  false: the device's or the library's refusal.
bool match_bank(MatchRun &run, syldet_t *h, syldet_recordings_t *r, const float *rows, int64_t row_samples, int64_t stride, int C, int D, hipStream_t stream,
                std::vector<std::vector<int64_t>> &events)
{
    const size_t N = (size_t)run.C * (size_t)D;             // tables: a class's detectors one after another
    events.assign(N, {});
    const int64_t J = std::max<int64_t>(0, syldet_count_frames(h, row_samples));
    if (J <= 0 || D <= 0) return true;
    syldet_matcher_bank_t *m = nullptr;
    // (files of one length: the uniform bank, whose matches and bytes are what they were)
    int st = run.ragged ? syldet_matcher_bank_create_ragged(h, r, run.templ.data(), run.K, run.tn.data(), run.bins, run.ta.data(), run.tclass.data(), run.C, &m)
                        : syldet_matcher_bank_create(h, r, run.templ.data(), run.K, run.n, run.bins, run.anchor, run.tclass.data(), run.C, &m);
    const bool each = std::adjacent_find(run.separations.begin(), run.separations.end(), std::not_equal_to<int32_t>()) != run.separations.end();
    DevBuf d_cols, d_scores, d_events, d_counts;
    bool ok = true;
    std::vector<int64_t> counts(N, 0), table;
    int64_t cap = 1024;
    if (!st) {
        ok = d_cols.alloc((size_t)C * (size_t)J * (size_t)run.bins * sizeof(float)) && d_scores.alloc((size_t)run.C * (size_t)C * (size_t)J * sizeof(float)) &&
             d_counts.alloc(N * sizeof(int64_t));
        if (ok) st = syldet_spectrogram_device(h, rows, row_samples, stride, (float *)d_cols.p, stream);
        if (ok && !st) st = syldet_match_bank_scores_device(m, (const float *)d_cols.p, J, 0, (float *)d_scores.p, nullptr, stream);
        for (int pass = 0; ok && !st && pass < 2; pass++) {
            DevBuf d_table;
            ok = d_table.alloc(N * (size_t)cap * sizeof(int64_t));
            if (ok && each)
                st = syldet_match_bank_peaks_each_device(m, (const float *)d_scores.p, nullptr, J, run.thresholds.data(), run.separations.data(),
                                                         (int64_t *)d_table.p, cap, (int64_t *)d_counts.p, nullptr, nullptr, stream);
            else if (ok)
                st = syldet_match_bank_peaks_device(m, (const float *)d_scores.p, nullptr, J, run.thresholds.data(), run.separations[0], (int64_t *)d_table.p, cap,
                                                    (int64_t *)d_counts.p, nullptr, nullptr, stream);
            table.assign(N * (size_t)cap, 0);
            if (ok && !st)
                ok = hipMemcpyAsync(counts.data(), d_counts.p, counts.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream) == hipSuccess &&
                     hipMemcpyAsync(table.data(), d_table.p, table.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream) == hipSuccess &&
                     hipStreamSynchronize(stream) == hipSuccess;
            const int64_t most = *std::max_element(counts.begin(), counts.end());
            if (most <= cap) break;
            cap = most;                                     // a table too small: once more with the largest count
        }
    }
    syldet_matcher_bank_destroy(m);
    if (st) std::fprintf(stderr, "Unable to match the template: %s: %s\n", syldet_strerror(st), syldet_last_error());
    if (!ok || st) return false;
    for (size_t d = 0; d < N; d++) events[d].assign(table.begin() + d * (size_t)cap, table.begin() + d * (size_t)cap + (size_t)std::min(counts[d], cap));
    return true;
}

// one file's lines, class by class: its tracks are the bank's detectors k0 .. k0 + tracks - 1 of D (events: match_bank's; a bank that
// failed has none)
void match_add_file(MatchRun &run, const std::string &path, const std::vector<std::vector<int64_t>> &events, size_t k0, int tracks, size_t D)
{
    if (events.size() != (size_t)run.C * D) return;
    for (size_t c = 0; c < (size_t)run.C; c++)
        for (size_t t = 0; t < (size_t)tracks && k0 + t < D; t++)
            for (const int64_t s : events[c * D + k0 + t]) run.lines[c] += path + "\t" + std::to_string(t) + "\t" + std::to_string(s) + "\n";
}

// the files, behind the last audio file: class i's matches in the i-th --match-out
bool match_finish(const MatchRun &run)
{
    bool all = true;
    for (size_t c = 0; c < (size_t)run.C; c++) {
        const std::string &out = run.opt.out_paths[c];
        FILE *f = std::fopen(out.c_str(), "wb");
        bool ok = f != nullptr && std::fwrite(run.lines[c].data(), 1, run.lines[c].size(), f) == run.lines[c].size();
        if (f && std::fclose(f) != 0) ok = false;
        if (!ok) std::fprintf(stderr, "Unable to write %s.\n", out.c_str());
        all = all && ok;
    }
    return all && !run.failed;
}

}  // namespace
