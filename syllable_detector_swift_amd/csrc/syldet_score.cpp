// syldet_score.cpp -- threshold calibration (include/syldet.h, "threshold calibration"): the scorer that keeps thresholds, labels
// and a packed plan's slots on the device so that syldet_score_device is one launch (kernels_score.hip), the same scan on the
// host (score_scan.hpp, one threshold after another), and the choice of a threshold from the tables.
#include <limits>

#include "score_scan.hpp"
#include "syldet_handle.hpp"

static_assert(SYLDET_SCORE_COLUMNS == sd::kScoreColumns && SYLDET_SCORE_DETECTIONS == sd::kScoreDetections && SYLDET_SCORE_HITS == sd::kScoreHits &&
              SYLDET_SCORE_FALSE_POSITIVES == sd::kScoreFalsePositives && SYLDET_SCORE_REPEATS == sd::kScoreRepeats &&
              SYLDET_SCORE_SUM_OFFSET == sd::kScoreSumOffset && SYLDET_SCORE_SUM_OFFSET_SQUARED == sd::kScoreSumOffsetSquared,
              "the header's columns are the scan's");

struct syldet_scorer : sd::DetectorTable {  // (the spans: evaluations)
    int64_t n_labels = 0;
    sd::DeviceBuffer d_blob;                 // thresholds | group_least | label_begin | labels | spans
    sd::ScoreDesc desc{};
};

namespace {

constexpr int64_t kFrameLimit = (int64_t)1 << 62;

int check_thresholds(const double *thresholds, int32_t K)
{
    if (K < 1 || K > SYLDET_SCORE_MAX_THRESHOLDS)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_thresholds must be in [1, " + std::to_string(SYLDET_SCORE_MAX_THRESHOLDS) + "]");
    if (!thresholds) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL thresholds");
    for (int32_t k = 0; k < K; k++)
        if (std::isnan(thresholds[k])) return fail(SYLDET_ERR_INVALID_ARGUMENT, "thresholds[" + std::to_string(k) + "] is NaN");
    return SYLDET_OK;
}

int check_tolerance(int64_t m)
{
    if (m < 0 || m > SYLDET_SCORE_MAX_TOLERANCE)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "tolerance_samples must be in [0, " + std::to_string(SYLDET_SCORE_MAX_TOLERANCE) + "]");
    return SYLDET_OK;
}

// one detector's labels: sorted, their windows disjoint (t_{j+1} - t_j > 2 m; the difference of two sorted int64 fits uint64)
int check_labels(const int64_t *t, int64_t n, int64_t m, int64_t detector)
{
    for (int64_t j = 0; j + 1 < n; j++)
        if (t[j + 1] <= t[j] || (uint64_t)t[j + 1] - (uint64_t)t[j] <= (uint64_t)(2 * m))
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "detector " + std::to_string(detector) + ", label " + std::to_string(j + 1) + " (sample " +
                        std::to_string(t[j + 1]) + "): not more than 2 x tolerance behind label " + std::to_string(j) + " (sample " +
                        std::to_string(t[j]) + "); the labels are sorted and their windows disjoint");
    return SYLDET_OK;
}

}  // namespace

extern "C" {

int syldet_scorer_create(const syldet_t *h, const syldet_recordings_t *r, const double *thresholds, int32_t n_thresholds,
                         const int64_t *labels, const int64_t *label_begin, int64_t tolerance_samples, double debounce_seconds,
                         syldet_scorer_t **out)
{
    if (!out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (int st = check_thresholds(thresholds, n_thresholds)) return st;
    if (int st = check_tolerance(tolerance_samples)) return st;
    if (!label_begin) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL label_begin");
    std::unique_ptr<syldet_scorer, int (*)(syldet_scorer_t *)> s(nullptr, syldet_scorer_destroy);
    try {
        s.reset(new syldet_scorer());
        if (int st = s->read(h, r, sd::kSpanEvals)) return st;
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    const sd::BankInfo &b = s->bank;
    const int32_t D = s->D;
    const double frames = debounce_seconds * b.sampling_rate;            // TrackDetector.swift:19-26
    if (!(std::fabs(frames) < (double)kFrameLimit)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "debounce_seconds x samplingRate is not a number below 2^62");
    if (label_begin[0] != 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "label_begin[0] must be 0");
    for (int32_t d = 0; d < D; d++)
        if (label_begin[d + 1] < label_begin[d]) return fail(SYLDET_ERR_INVALID_ARGUMENT, "label_begin[" + std::to_string(d + 1) + "] decreases");
    const int64_t n_labels = label_begin[D];
    if (n_labels > 0 && !labels) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL labels");
    for (int32_t d = 0; d < D; d++)
        if (int st = check_labels(labels + label_begin[d], label_begin[d + 1] - label_begin[d], tolerance_samples, d)) return st;
    const int K = n_thresholds, groups = (K + 63) / 64;
    if ((int64_t)D * groups > 0x7fffffff) return fail(SYLDET_ERR_UNSUPPORTED, "more than 2^31 - 1 (detector, group of 64 thresholds) pairs");

    std::vector<float> thr, least;
    try {
        thr.resize((size_t)K);
        least.assign((size_t)groups, std::numeric_limits<float>::infinity());
        for (int k = 0; k < K; k++) {
            thr[(size_t)k] = sd::score_threshold_f32(thresholds[k]);
            least[(size_t)(k / 64)] = std::fmin(least[(size_t)(k / 64)], thr[(size_t)k]);
        }
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    s->n_labels = n_labels;
    sd::Carver blob;
    const size_t at_thr = blob.take(bytes_of(thr)), at_least = blob.take(bytes_of(least)), at_begin = blob.take(((size_t)D + 1) * sizeof(int64_t)),
                 at_labels = blob.take((size_t)n_labels * sizeof(int64_t)), at_spans = blob.take(bytes_of(s->spans));
    SYLDET_HIP(hipSetDevice(b.device));
    if (int st = s->d_blob.reserve(blob.total + 16)) return st;
    char *base = (char *)s->d_blob.ptr;
    SYLDET_HIP(upload(base, at_thr, thr));
    SYLDET_HIP(upload(base, at_least, least));
    SYLDET_HIP(upload(base, at_begin, label_begin, ((size_t)D + 1) * sizeof(int64_t)));
    SYLDET_HIP(upload(base, at_labels, labels, (size_t)n_labels * sizeof(int64_t)));
    SYLDET_HIP(upload(base, at_spans, s->spans));
    s->desc = sd::ScoreDesc{(const float *)(base + at_thr),
                            (const float *)(base + at_least),
                            (const int64_t *)(base + at_labels),
                            (const int64_t *)(base + at_begin),
                            r ? (const sd::DetSpan *)(base + at_spans) : nullptr,
                            K,
                            tolerance_samples,
                            (int64_t)frames};
    *out = s.release();
    return SYLDET_OK;
}

int syldet_scorer_destroy(syldet_scorer_t *s)
{
    if (!s) return SYLDET_OK;
    if (s->d_blob.ptr) (void)hipSetDevice(s->bank.device);
    s->d_blob.release();
    delete s;
    return SYLDET_OK;
}

int syldet_scorer_shape(const syldet_scorer_t *s, int32_t *n_detectors, int32_t *n_thresholds, int64_t *n_labels)
{
    if (!s) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_detectors) *n_detectors = s->D;
    if (n_thresholds) *n_thresholds = s->desc.K;
    if (n_labels) *n_labels = s->n_labels;
    return SYLDET_OK;
}

int syldet_score_device(syldet_scorer_t *s, const float *d_outputs, int64_t n_evals, int32_t output, int64_t *d_table, void *hip_stream)
{
    if (!s || !d_outputs || !d_table) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_evals < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_evals is negative");
    if (output < 0 || output >= s->bank.geom.outputs)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "output " + std::to_string(output) + " outside [0, " + std::to_string(s->bank.geom.outputs) + ")");
    if (int st = s->row_units_arg(n_evals, "n_evals", "evaluations")) return st;
    if (s->D == 0) return SYLDET_OK;
    SYLDET_HIP(hipSetDevice(s->bank.device));
    SYLDET_HIP(sd::launch_score(s->desc, s->D, d_outputs, n_evals, s->bank.geom.outputs, output, s->bank.geom.first_index, s->bank.geom.hop, d_table,
                                (hipStream_t)hip_stream));
    return SYLDET_OK;
}

int syldet_score_host(const float *values, int64_t n_evals, int64_t value_stride, const double *thresholds, int32_t n_thresholds,
                      const int64_t *labels, int64_t n_labels, int64_t tolerance_samples, int64_t first_index, int64_t hop,
                      int64_t debounce_frames, int64_t *table)
{
    if (int st = check_thresholds(thresholds, n_thresholds)) return st;
    if (int st = check_tolerance(tolerance_samples)) return st;
    if (!table || n_evals < 0 || (n_evals > 0 && !values) || value_stride < 1 || n_labels < 0 || (n_labels > 0 && !labels))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "a NULL array, a negative count or a stride below 1");
    // (sample numbers stay below 2^62: nothing in the scan can overflow)
    if (hop < 1 || hop > ((int64_t)1 << 30) || n_evals > ((int64_t)1 << 31) || first_index <= -kFrameLimit / 2 || first_index >= kFrameLimit / 2 ||
        debounce_frames <= -kFrameLimit || debounce_frames >= kFrameLimit)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "hop outside [1, 2^30], more than 2^31 evaluations, or first_index / debounce_frames out of range");
    if (int st = check_labels(labels, n_labels, tolerance_samples, 0)) return st;
    for (int32_t k = 0; k < n_thresholds; k++) {
        const float thr = sd::score_threshold_f32(thresholds[k]);
        sd::ScoreLane s;
        sd::ScoreCursor c = sd::score_cursor_start(labels, n_labels);
        for (int64_t e = 0; e < n_evals; e++) {
            const float v = values[e * value_stride];
            if (!(v >= thr)) continue;                                   // (the kernel visits what reaches its group's least threshold)
            sd::score_visit(s, true, first_index + e * hop, debounce_frames, labels, n_labels, tolerance_samples, c);
        }
        std::memcpy(table + (size_t)k * sd::kScoreColumns, s.n, sizeof(s.n));
    }
    return SYLDET_OK;
}

int syldet_score_choose(const int64_t *table, int32_t n_detectors, int32_t n_thresholds, const int64_t *n_labels,
                        double false_positive_cost, int32_t *best, int64_t *totals, double *costs)
{
    if (n_thresholds < 1 || n_thresholds > SYLDET_SCORE_MAX_THRESHOLDS)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_thresholds must be in [1, " + std::to_string(SYLDET_SCORE_MAX_THRESHOLDS) + "]");
    if (!best || n_detectors < 0 || (n_detectors > 0 && (!table || !n_labels)) || std::isnan(false_positive_cost))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "a NULL array, a negative count or a NaN cost");
    int64_t labelled = 0;
    for (int32_t d = 0; d < n_detectors; d++) {
        if (n_labels[d] < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_labels[" + std::to_string(d) + "] is negative");
        labelled += n_labels[d];
    }
    int32_t at = 0;
    double least = 0.0;
    for (int32_t k = 0; k < n_thresholds; k++) {
        int64_t sum[sd::kScoreColumns] = {0, 0, 0, 0, 0, 0};
        for (int32_t d = 0; d < n_detectors; d++)
            for (int c = 0; c < sd::kScoreColumns; c++) sum[c] += table[((size_t)d * (size_t)n_thresholds + (size_t)k) * sd::kScoreColumns + c];
        const double cost = (double)(labelled - sum[sd::kScoreHits]) + false_positive_cost * (double)(sum[sd::kScoreFalsePositives] + sum[sd::kScoreRepeats]);
        if (totals) std::memcpy(totals + (size_t)k * sd::kScoreColumns, sum, sizeof(sum));
        if (costs) costs[k] = cost;
        if (k == 0 || cost < least) {
            least = cost;
            at = k;
        }
    }
    *best = at;
    return SYLDET_OK;
}

}  // extern "C"
