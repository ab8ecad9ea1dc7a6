// --score: the labels file, what a run adds up over its batches, and the table written at the end.
#pragma once

#include <algorithm>
#include <cmath>
#include <map>

#include "options.hpp"

namespace {

using Labels = std::map<std::string, std::map<long, std::vector<int64_t>>>;   // file as -a names it -> track -> sorted samples

struct ScoreRun {
    std::vector<double> thresholds;
    int output = 0;
    int64_t tolerance = 0;                                  // samples
    Labels labels;
    std::vector<int64_t> totals;                            // [K][6], summed over every scored track
    int64_t n_labels = 0;                                   // ... and their labels
    bool failed = false;
};

// LABELS: lines of file<TAB>track<TAB>sample (the sample counted from the file's start, at the network's rate)
bool read_labels(const std::string &path, ScoreRun &run, std::string &err)
{
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { err = "unable to open " + path; return false; }
    std::string text;
    char buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
    std::fclose(f);
    size_t at = 0;
    for (long line = 1; at < text.size(); line++) {
        size_t end = text.find('\n', at);
        if (end == std::string::npos) end = text.size();
        std::string l = text.substr(at, end - at);
        at = end + 1;
        if (!l.empty() && l.back() == '\r') l.pop_back();
        if (l.empty() || l[0] == '#') continue;
        const size_t t2 = l.rfind('\t'), t1 = t2 == std::string::npos || t2 == 0 ? std::string::npos : l.rfind('\t', t2 - 1);
        char *e1 = nullptr, *e2 = nullptr;
        const std::string track = t1 == std::string::npos ? "" : l.substr(t1 + 1, t2 - t1 - 1), sample = t1 == std::string::npos ? "" : l.substr(t2 + 1);
        const long trk = std::strtol(track.c_str(), &e1, 10);
        const long long smp = std::strtoll(sample.c_str(), &e2, 10);
        if (t1 == std::string::npos || t1 == 0 || track.empty() || sample.empty() || *e1 || *e2 || trk < 0) {
            err = path + ", line " + std::to_string(line) + ": not file<TAB>track<TAB>sample";
            return false;
        }
        run.labels[l.substr(0, t1)][trk].push_back((int64_t)smp);
    }
    for (auto &file : run.labels)
        for (auto &track : file.second) std::sort(track.second.begin(), track.second.end());
    return true;
}

// the labels of one track of one file (none: an empty list)
const std::vector<int64_t> &labels_of(const Labels &labels, const std::string &path, long track)
{
    static const std::vector<int64_t> none;
    const auto of_file = labels.find(path);
    if (of_file == labels.end()) return none;
    const auto of_track = of_file->second.find(track);
    return of_track == of_file->second.end() ? none : of_track->second;
}

// TABLE: one line per threshold -- threshold detections hits misses false_positives repeats mean_offset sd_offset cost, tab
// separated, the offsets in samples (mean and deviation of the hits' offsets from the two sums, in double; nan without a hit) --
// and a last line "# best <threshold>" (syldet_score_choose: the lowest threshold of the smallest cost)
bool write_score_table(const ScoreOpt &opt, const ScoreRun &run)
{
    const int32_t K = (int32_t)run.thresholds.size();
    std::vector<double> costs((size_t)K);
    int32_t best = 0;
    if (int st = syldet_score_choose(run.totals.data(), 1, K, &run.n_labels, opt.cost, &best, nullptr, costs.data())) {
        std::fprintf(stderr, "Unable to choose a threshold: %s: %s\n", syldet_strerror(st), syldet_last_error());
        return false;
    }
    FILE *f = std::fopen(opt.out_path.c_str(), "wb");
    if (!f) {
        std::fprintf(stderr, "Unable to write %s.\n", opt.out_path.c_str());
        return false;
    }
    for (int32_t k = 0; k < K; k++) {
        const int64_t *t = run.totals.data() + (size_t)k * SYLDET_SCORE_COLUMNS;
        const int64_t hits = t[SYLDET_SCORE_HITS];
        std::fprintf(f, "%.17g\t%lld\t%lld\t%lld\t%lld\t%lld\t", run.thresholds[(size_t)k], (long long)t[SYLDET_SCORE_DETECTIONS], (long long)hits,
                     (long long)(run.n_labels - hits), (long long)t[SYLDET_SCORE_FALSE_POSITIVES], (long long)t[SYLDET_SCORE_REPEATS]);
        if (hits > 0) {
            const double mean = (double)t[SYLDET_SCORE_SUM_OFFSET] / (double)hits;
            const double square = mean * mean;              // (a statement of its own: no fused multiply-subtract below)
            const double var = (double)t[SYLDET_SCORE_SUM_OFFSET_SQUARED] / (double)hits - square;
            std::fprintf(f, "%.17g\t%.17g\t", mean, std::sqrt(var > 0.0 ? var : 0.0));
        } else {
            std::fputs("nan\tnan\t", f);
        }
        std::fprintf(f, "%.17g\n", costs[(size_t)k]);
    }
    std::fprintf(f, "# best %.17g\n", run.thresholds[(size_t)best]);
    return std::fclose(f) == 0;
}

}  // namespace
