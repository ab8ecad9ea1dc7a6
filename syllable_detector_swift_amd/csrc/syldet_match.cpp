// syldet_match.cpp -- template matching (include/syldet.h, "template matching"; kernels_match.hip): the matcher that keeps the
// normalised template and a packed plan's detectors on the device, so that syldet_match_scores_device and
// syldet_match_peaks_device are launches only; and the host functions (match_peaks.hpp: the rule the kernel runs).
// A bank of templates (syldet_matcher_bank_*, "template matching: a bank of templates") is the same matcher with K templates and a
// class table on the device; match_classes.hpp holds the rule of a class's score.  A ragged bank ("template matching: a ragged
// bank") is a bank whose templates have their own lengths and anchors: the same handle type, match_ragged.hpp its plan.

#include <limits>

#include "match_classes.hpp"
#include "match_peaks.hpp"
#include "match_ragged.hpp"
#include "syldet_handle.hpp"

static_assert(SYLDET_MATCH_MAX_TEMPLATE == sd::kMatchMaxTemplate && SYLDET_MATCH_MAX_SEPARATION == sd::kMatchMaxSeparation &&
                  SYLDET_MATCH_MAX_TEMPLATES == sd::kMatchMaxTemplates && SYLDET_MATCH_MAX_CLASSES == sd::kMatchMaxClasses,
              "the header's limits are the kernels'");

// what a matcher and a bank of templates share: the bank, the packed plan and the kernels' plan
struct MatcherCore : sd::DetectorTable {     // (the spans: frames)
    std::vector<float> templ;                // t^ [n][bins]; a bank of templates: [K][n][bins]
    sd::DeviceBuffer d_fixed;                // t^ | (a bank's tables) | by_det [D] | by_row [D] | row_begin [rows + 1]
    sd::MatchDesc desc{};
    ~MatcherCore()
    {
        if (d_fixed.ptr) (void)hipSetDevice(bank.device);
        d_fixed.release();
    }
};

struct syldet_matcher : MatcherCore {};

struct syldet_matcher_bank : MatcherCore {
    std::vector<int32_t> tclass;             // [K]
    std::vector<int32_t> tn, ta;             // [K] every template's frames and anchor (a uniform bank: K times the same)
    sd::MatchBankDesc b{};                   // a ragged bank: the peaks kernels' (planes indexed by the anchor: n 1, anchor 0)
    bool ragged = false;
    sd::MatchRaggedDesc rg{};
};

namespace {

int template_args(const float *templ, int64_t n, int64_t bins)
{
    if (!templ) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL template");
    if (n < 1 || bins < 1 || n * bins > SYLDET_MATCH_MAX_TEMPLATE || n > SYLDET_MATCH_MAX_TEMPLATE || bins > SYLDET_MATCH_MAX_TEMPLATE)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "a template of " + std::to_string(n) + " x " + std::to_string(bins) + " elements is outside [1, " +
                                                     std::to_string(SYLDET_MATCH_MAX_TEMPLATE) + "]");
    return SYLDET_OK;
}

// t^ = fp32(t / ||t||_2), the norm and the division in fp64
int normalise(const float *templ, int n, int bins, float *out)
{
    double sq = 0.0;
    for (int k = 0; k < n * bins; k++) {
        if (!std::isfinite(templ[k])) return fail(SYLDET_ERR_INVALID_ARGUMENT, "template element " + std::to_string(k) + " is not finite");
        sq += (double)templ[k] * (double)templ[k];
    }
    if (sq == 0.0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "the template is all zero");
    const double norm = std::sqrt(sq);
    for (int k = 0; k < n * bins; k++) out[k] = (float)((double)templ[k] / norm);
    return SYLDET_OK;
}

int peaks_args(float threshold, int32_t separation, int64_t capacity)
{
    if (threshold != threshold) return fail(SYLDET_ERR_INVALID_ARGUMENT, "the threshold is NaN");
    if (separation < 0 || separation > SYLDET_MATCH_MAX_SEPARATION)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "separation " + std::to_string(separation) + " is outside [0, " + std::to_string(SYLDET_MATCH_MAX_SEPARATION) + "]");
    if (capacity < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "capacity is negative");
    return SYLDET_OK;
}

// Everything of a matcher behind its arguments' own rules: the bank's checks, t^ of each of the K templates, the packed plan, the
// kernels' plan, and t^ | tables | by_det | by_row | row_begin on the device (*d_tables: where `tables` lies there).
// lens: NULL (K templates of n frames), or a ragged bank's lengths, n the greatest and *plan its tile.
int core_create(MatcherCore *m, const syldet_t *h, const syldet_recordings_t *r, const float *templates, int K, int32_t n, int32_t bins, int32_t anchor,
                const std::vector<int32_t> &tables, const int32_t **d_tables, const int32_t *lens = nullptr, const sd::MatchRaggedPlan *plan = nullptr)
{
    if (h->classes.size() > 1) return fail(SYLDET_ERR_UNSUPPORTED, "columns of a mixed bank: its classes' columns are ragged");
    sd::BankInfo b{};
    sd::bank_info(h, &b);
    if (bins != b.geom.bins)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "the template has " + std::to_string(bins) + " bins, the bank's columns " + std::to_string(b.geom.bins));
    if (anchor < 0) anchor = n - 1;
    if (anchor >= n) return fail(SYLDET_ERR_INVALID_ARGUMENT, "anchor " + std::to_string(anchor) + " is outside [0, " + std::to_string(n) + ")");

    std::vector<sd::DetSpan> by_row;
    std::vector<int32_t> row_begin;
    try {
        size_t all = 0;
        for (int k = 0; k < K; k++) all += (size_t)(lens ? lens[k] : n) * bins;
        m->templ.assign(all, 0.0f);
        for (size_t k = 0, at = 0; k < (size_t)K; k++) {
            const int nk = lens ? lens[k] : n;
            if (int st = normalise(templates + at, nk, bins, m->templ.data() + at)) return st;
            at += (size_t)nk * bins;
        }
        if (int st = m->read(h, r, sd::kSpanFrames)) return st;
        if (r) sd::spans_by_row(m->spans, b.channels, &by_row, &row_begin);
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    const int D = m->D;
    sd::MatchDesc &d = m->desc;
    d.rows = b.channels;
    d.D = D;
    d.n = n;
    d.bins = bins;
    d.anchor = anchor;
    d.origin = (int64_t)b.geom.gap + b.window_length;       // syldet_align_anchor(COLUMNS)
    d.hop = b.geom.hop;
    sd::match_plan(d);
    if (plan) {
        d.matrix = plan->matrix;
        d.lds_bytes = plan->lds_bytes;
    }
    // (measurement only, tools/match_timing.py: the plain form on a shape the matrix form takes)
    if (const char *e = std::getenv("SYLDET_MATCH_PLAIN"))
        if (e[0] == '1') d.matrix = 0;

    sd::Carver blob;
    const size_t at_t = blob.take(bytes_of(m->templ)), at_x = blob.take(bytes_of(tables)), at_det = blob.take(bytes_of(m->spans)),
                 at_row = blob.take(bytes_of(by_row)), at_begin = blob.take(bytes_of(row_begin));
    SYLDET_HIP(hipSetDevice(b.device));
    SYLDET_HIP(sd::match_prepare());
    if (d_tables) SYLDET_HIP(sd::match_bank_prepare());
    if (int st = m->d_fixed.reserve(blob.total + 16)) return st;
    char *base = (char *)m->d_fixed.ptr;
    SYLDET_HIP(upload(base, at_t, m->templ));
    SYLDET_HIP(upload(base, at_x, tables));
    SYLDET_HIP(upload(base, at_det, m->spans));
    SYLDET_HIP(upload(base, at_row, by_row));
    SYLDET_HIP(upload(base, at_begin, row_begin));
    d.templ = (const float *)(base + at_t);
    if (d_tables) *d_tables = (const int32_t *)(base + at_x);
    d.by_det = r ? (const sd::DetSpan *)(base + at_det) : nullptr;
    d.by_row = r ? (const sd::DetSpan *)(base + at_row) : nullptr;
    d.row_begin = r ? (const int32_t *)(base + at_begin) : nullptr;
    return SYLDET_OK;
}

// what the two scores calls ask of n_frames and row_stride (0: the rows lie end to end)
int scores_args(const MatcherCore *m, int64_t n_frames, int64_t &row_stride)
{
    if (n_frames < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_frames is negative");
    if (int st = m->row_units_arg(n_frames, "n_frames", "frames")) return st;
    if (n_frames > ((int64_t)1 << 40) / m->desc.bins) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_frames x bins is above 2^40");
    if (row_stride == 0) row_stride = n_frames * m->desc.bins;
    if (row_stride < n_frames * m->desc.bins)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "row_stride " + std::to_string(row_stride) + " is below the " + std::to_string(n_frames * m->desc.bins) +
                                                     " elements of a row");
    return SYLDET_OK;
}

// K and C of a bank (n_classes: K where there is no table)
int bank_count_args(int32_t n_templates, const int32_t *template_class, int32_t &n_classes)
{
    if (n_templates < 1 || n_templates > SYLDET_MATCH_MAX_TEMPLATES)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, std::to_string(n_templates) + " templates are outside [1, " + std::to_string(SYLDET_MATCH_MAX_TEMPLATES) + "]");
    if (!template_class) {
        if (n_classes != 0 && n_classes != n_templates)
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "without a class table there are as many classes as templates (or 0 for that number)");
        n_classes = n_templates;
    }
    if (n_classes < 1 || n_classes > SYLDET_MATCH_MAX_CLASSES)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, std::to_string(n_classes) + " classes are outside [1, " + std::to_string(SYLDET_MATCH_MAX_CLASSES) + "]");
    return SYLDET_OK;
}

// the handle with its class table, and the tables that go to the device: order [K], the templates class by class, ascending k within
// a class; then the class of each
int bank_begin(std::unique_ptr<syldet_matcher_bank> &m, int K, const int32_t *template_class, int32_t n_classes, std::vector<int32_t> &tables)
{
    try {
        m.reset(new syldet_matcher_bank());
        m->tclass.resize((size_t)K);
        std::vector<int> members((size_t)n_classes, 0);
        for (int k = 0; k < K; k++) {
            const int32_t c = template_class ? template_class[k] : k;
            if (c < 0 || c >= n_classes)
                return fail(SYLDET_ERR_INVALID_ARGUMENT, "template " + std::to_string(k) + "'s class " + std::to_string(c) + " is outside [0, " +
                                                             std::to_string(n_classes) + ")");
            m->tclass[(size_t)k] = c;
            members[(size_t)c]++;
        }
        for (int c = 0; c < n_classes; c++)
            if (!members[(size_t)c]) return fail(SYLDET_ERR_INVALID_ARGUMENT, "class " + std::to_string(c) + " has no template");
        for (int c = 0; c < n_classes; c++)
            for (int k = 0; k < K; k++)
                if (m->tclass[(size_t)k] == c) tables.push_back(k);
        for (int i = 0; i < K; i++) tables.push_back(m->tclass[(size_t)tables[(size_t)i]]);
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    return SYLDET_OK;
}

// what the bank's two peaks calls ask behind their thresholds and separations
int bank_peaks_args(const syldet_matcher_bank *m, const float *d_scores, const int32_t *d_which, int64_t n_frames, const int64_t *d_events, int64_t capacity,
                    const int64_t *d_counts, const int32_t *d_event_template)
{
    if (d_event_template && !d_which) return fail(SYLDET_ERR_INVALID_ARGUMENT, "d_event_template needs d_which");
    if (n_frames < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_frames is negative");
    if (int st = m->row_units_arg(n_frames, "n_frames", "frames")) return st;
    if (m->D > 0 && (!d_counts || (n_frames > 0 && !d_scores) || (capacity > 0 && !d_events))) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    return SYLDET_OK;
}

}  // namespace

extern "C" {

int syldet_matcher_create(const syldet_t *h, const syldet_recordings_t *r, const float *templ, int32_t n, int32_t bins, int32_t anchor,
                          syldet_matcher_t **out)
{
    if (!out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (int st = template_args(templ, n, bins)) return st;
    std::unique_ptr<syldet_matcher> m;
    try {
        m.reset(new syldet_matcher());
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    if (int st = core_create(m.get(), h, r, templ, 1, n, bins, anchor, {}, nullptr)) return st;
    *out = m.release();
    return SYLDET_OK;
}

int syldet_matcher_destroy(syldet_matcher_t *m)
{
    delete m;
    return SYLDET_OK;
}

int syldet_matcher_shape(const syldet_matcher_t *m, int32_t *n_detectors, int32_t *n, int32_t *bins, int32_t *anchor, int32_t *matrix_form)
{
    if (!m) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_detectors) *n_detectors = m->D;
    if (n) *n = m->desc.n;
    if (bins) *bins = m->desc.bins;
    if (anchor) *anchor = m->desc.anchor;
    if (matrix_form) *matrix_form = m->desc.matrix;
    return SYLDET_OK;
}

int syldet_matcher_template(const syldet_matcher_t *m, float *t_hat)
{
    if (!m || !t_hat) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    std::memcpy(t_hat, m->templ.data(), m->templ.size() * sizeof(float));
    return SYLDET_OK;
}

int syldet_match_scores_device(syldet_matcher_t *m, const float *d_columns, int64_t n_frames, int64_t row_stride, float *d_scores, void *hip_stream)
{
    if (!m) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (int st = scores_args(m, n_frames, row_stride)) return st;
    if (n_frames > 0 && (!d_columns || !d_scores)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_frames == 0) return SYLDET_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    SYLDET_HIP(hipSetDevice(m->bank.device));
    m->h->prof_begin();
    KernelTimer t(m->h, stream, m->desc.matrix ? "match_scores_mfma_kernel" : "match_scores_plain_kernel");
    SYLDET_HIP(sd::launch_match_scores(m->desc, d_columns, n_frames, row_stride, d_scores, stream));
    return SYLDET_OK;
}

int syldet_match_peaks_device(syldet_matcher_t *m, const float *d_scores, int64_t n_frames, float threshold, int32_t separation, int64_t *d_events,
                              int64_t capacity, int64_t *d_counts, float *d_event_scores, void *hip_stream)
{
    if (!m) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (int st = peaks_args(threshold, separation, capacity)) return st;
    if (n_frames < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_frames is negative");
    if (int st = m->row_units_arg(n_frames, "n_frames", "frames")) return st;
    if (m->D > 0 && (!d_counts || (n_frames > 0 && !d_scores) || (capacity > 0 && !d_events))) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (m->D == 0) return SYLDET_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    SYLDET_HIP(hipSetDevice(m->bank.device));
    m->h->prof_begin();
    KernelTimer t(m->h, stream, "match_peaks_kernel");
    SYLDET_HIP(sd::launch_match_peaks(m->desc, d_scores, n_frames, threshold, separation, d_events, capacity, d_counts, d_event_scores, stream));
    return SYLDET_OK;
}

// ---- a bank of templates ----
int syldet_matcher_bank_create(const syldet_t *h, const syldet_recordings_t *r, const float *templates, int32_t n_templates, int32_t n, int32_t bins,
                               int32_t anchor, const int32_t *template_class, int32_t n_classes, syldet_matcher_bank_t **out)
{
    if (!out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (int st = bank_count_args(n_templates, template_class, n_classes)) return st;
    if (int st = template_args(templates, n, bins)) return st;
    const int K = n_templates;
    std::unique_ptr<syldet_matcher_bank> m;
    std::vector<int32_t> tables;
    if (int st = bank_begin(m, K, template_class, n_classes, tables)) return st;
    try {
        m->tn.assign((size_t)K, n);
        m->ta.assign((size_t)K, anchor < 0 ? n - 1 : anchor);
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    const int32_t *d_tables = nullptr;
    if (int st = core_create(m.get(), h, r, templates, K, n, bins, anchor, tables, &d_tables)) return st;
    m->b.d = m->desc;
    m->b.order = d_tables;
    m->b.order_class = d_tables + K;
    m->b.K = K;
    m->b.C = n_classes;
    *out = m.release();
    return SYLDET_OK;
}

int syldet_matcher_bank_destroy(syldet_matcher_bank_t *m)
{
    delete m;
    return SYLDET_OK;
}

int syldet_matcher_bank_shape(const syldet_matcher_bank_t *m, int32_t *n_detectors, int32_t *n_templates, int32_t *n_classes, int32_t *n, int32_t *bins,
                              int32_t *anchor, int32_t *matrix_form)
{
    if (!m) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_detectors) *n_detectors = m->D;
    if (n_templates) *n_templates = m->b.K;
    if (n_classes) *n_classes = m->b.C;
    if (n) *n = m->desc.n;
    if (bins) *bins = m->desc.bins;
    if (anchor) *anchor = m->desc.anchor;
    if (matrix_form) *matrix_form = m->desc.matrix;
    return SYLDET_OK;
}

int syldet_matcher_bank_templates(const syldet_matcher_bank_t *m, float *t_hat, int32_t *template_class)
{
    if (!m) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (t_hat) std::memcpy(t_hat, m->templ.data(), m->templ.size() * sizeof(float));
    if (template_class) std::memcpy(template_class, m->tclass.data(), m->tclass.size() * sizeof(int32_t));
    return SYLDET_OK;
}

int syldet_match_bank_scores_device(syldet_matcher_bank_t *m, const float *d_columns, int64_t n_frames, int64_t row_stride, float *d_scores,
                                    int32_t *d_which, void *hip_stream)
{
    if (!m) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (int st = scores_args(m, n_frames, row_stride)) return st;
    if (n_frames > 0 && (!d_columns || !d_scores)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_frames == 0) return SYLDET_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    SYLDET_HIP(hipSetDevice(m->bank.device));
    m->h->prof_begin();
    if (m->ragged) {
        KernelTimer t(m->h, stream, m->desc.matrix ? "match_ragged_scores_mfma_kernel" : "match_ragged_scores_plain_kernel");
        SYLDET_HIP(sd::launch_match_ragged_scores(m->rg, d_columns, n_frames, row_stride, d_scores, d_which, stream));
        return SYLDET_OK;
    }
    KernelTimer t(m->h, stream, m->desc.matrix ? "match_bank_scores_mfma_kernel" : "match_bank_scores_plain_kernel");
    SYLDET_HIP(sd::launch_match_bank_scores(m->b, d_columns, n_frames, row_stride, d_scores, d_which, stream));
    return SYLDET_OK;
}

int syldet_match_bank_peaks_device(syldet_matcher_bank_t *m, const float *d_scores, const int32_t *d_which, int64_t n_frames, const float *thresholds,
                                   int32_t separation, int64_t *d_events, int64_t capacity, int64_t *d_counts, float *d_event_scores,
                                   int32_t *d_event_template, void *hip_stream)
{
    if (!m) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (!thresholds) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL thresholds");
    for (int c = 0; c < m->b.C; c++)
        if (int st = peaks_args(thresholds[c], separation, capacity)) return st;
    if (int st = bank_peaks_args(m, d_scores, d_which, n_frames, d_events, capacity, d_counts, d_event_template)) return st;
    if (m->D == 0) return SYLDET_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    SYLDET_HIP(hipSetDevice(m->bank.device));
    m->h->prof_begin();
    KernelTimer t(m->h, stream, "match_bank_peaks_kernel");
    SYLDET_HIP(sd::launch_match_bank_peaks(m->b, d_scores, d_which, n_frames, thresholds, separation, d_events, capacity, d_counts, d_event_scores,
                                           capacity > 0 ? d_event_template : nullptr, stream));
    return SYLDET_OK;
}

// ---- a ragged bank ----
int syldet_matcher_bank_create_ragged(const syldet_t *h, const syldet_recordings_t *r, const float *templates, int32_t n_templates,
                                      const int32_t *template_n, int32_t bins, const int32_t *template_anchor, const int32_t *template_class,
                                      int32_t n_classes, syldet_matcher_bank_t **out)
{
    if (!out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (int st = bank_count_args(n_templates, template_class, n_classes)) return st;
    if (!template_n) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL template_n");
    const int K = n_templates;
    int32_t n_max = 0;
    for (int k = 0; k < K; k++) {
        if (int st = template_args(templates, template_n[k], bins)) return st;
        const int32_t a = template_anchor ? template_anchor[k] : template_n[k] - 1;
        if (a < 0 || a >= template_n[k])
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "template " + std::to_string(k) + "'s anchor " + std::to_string(a) + " is outside [0, " +
                                                         std::to_string(template_n[k]) + ")");
        n_max = std::max(n_max, template_n[k]);
    }
    std::unique_ptr<syldet_matcher_bank> m;
    std::vector<int32_t> tables;
    if (int st = bank_begin(m, K, template_class, n_classes, tables)) return st;
    sd::MatchRaggedPlan plan{};
    try {
        m->tn.assign(template_n, template_n + K);
        m->ta.resize((size_t)K);
        for (int k = 0; k < K; k++) m->ta[(size_t)k] = template_anchor ? template_anchor[k] : template_n[k] - 1;
        plan = sd::match_ragged_plan(m->tn.data(), m->ta.data(), K, bins);
        // the reads of a pass and of an energy sum lie in the staged frames [0, G)
        for (int k = 0; k < K; k++)
            if (sd::match_ragged_first(plan, m->ta[(size_t)k]) < 0 || sd::match_ragged_last(plan, m->tn[(size_t)k], m->ta[(size_t)k]) > plan.G - 1)
                return fail(SYLDET_ERR_INVALID_ARGUMENT, "a ragged bank's tile does not hold template " + std::to_string(k) + "'s windows");
        // ... behind order and order_class: every template's frames, anchor and first element in the concatenated t^
        tables.insert(tables.end(), m->tn.begin(), m->tn.end());
        tables.insert(tables.end(), m->ta.begin(), m->ta.end());
        int32_t at = 0;
        for (int k = 0; k < K; k++) {
            tables.push_back(at);
            at += m->tn[(size_t)k] * bins;
        }
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    const int32_t *d_tables = nullptr;
    if (int st = core_create(m.get(), h, r, templates, K, n_max, bins, 0, tables, &d_tables, m->tn.data(), &plan)) return st;
    m->ragged = true;
    sd::MatchRaggedDesc &g = m->rg;
    g.d = m->desc;
    g.order = d_tables;
    g.order_class = d_tables + K;
    g.len = d_tables + 2 * K;
    g.anchor = d_tables + 3 * K;
    g.offset = d_tables + 4 * K;
    g.K = K;
    g.C = n_classes;
    g.a_max = plan.a_max;
    g.G = plan.G;
    // the peaks kernels' view: every element of a detector is a position of its own, and the plane's index is the anchor frame
    m->b.d = m->desc;
    m->b.d.n = 1;
    m->b.d.anchor = 0;
    m->b.order = g.order;
    m->b.order_class = g.order_class;
    m->b.K = K;
    m->b.C = n_classes;
    *out = m.release();
    return SYLDET_OK;
}

int syldet_matcher_bank_lengths(const syldet_matcher_bank_t *m, int32_t *template_n, int32_t *template_anchor, int32_t *ragged)
{
    if (!m) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (template_n) std::memcpy(template_n, m->tn.data(), m->tn.size() * sizeof(int32_t));
    if (template_anchor) std::memcpy(template_anchor, m->ta.data(), m->ta.size() * sizeof(int32_t));
    if (ragged) *ragged = m->ragged ? 1 : 0;
    return SYLDET_OK;
}

int syldet_match_bank_peaks_each_device(syldet_matcher_bank_t *m, const float *d_scores, const int32_t *d_which, int64_t n_frames, const float *thresholds,
                                        const int32_t *separations, int64_t *d_events, int64_t capacity, int64_t *d_counts, float *d_event_scores,
                                        int32_t *d_event_template, void *hip_stream)
{
    if (!m) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (!thresholds) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL thresholds");
    if (!separations) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL separations");
    for (int c = 0; c < m->b.C; c++)
        if (int st = peaks_args(thresholds[c], separations[c], capacity)) return st;
    if (int st = bank_peaks_args(m, d_scores, d_which, n_frames, d_events, capacity, d_counts, d_event_template)) return st;
    if (m->D == 0) return SYLDET_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    SYLDET_HIP(hipSetDevice(m->bank.device));
    m->h->prof_begin();
    KernelTimer t(m->h, stream, "match_bank_peaks_each_kernel");
    SYLDET_HIP(sd::launch_match_bank_peaks_each(m->b, d_scores, d_which, n_frames, thresholds, separations, d_events, capacity, d_counts, d_event_scores,
                                                capacity > 0 ? d_event_template : nullptr, stream));
    return SYLDET_OK;
}

int syldet_match_classes_host(const float *template_scores, int64_t n_positions, int32_t n_templates, const int32_t *template_class, int32_t n_classes,
                              float *class_scores, int32_t *which)
{
    if (int st = bank_count_args(n_templates, template_class, n_classes)) return st;
    if (n_positions < 0 || (n_positions > 0 && (!template_scores || !class_scores))) return fail(SYLDET_ERR_INVALID_ARGUMENT, "a NULL array or a negative count");
    uint32_t members = 0;
    for (int k = 0; k < n_templates; k++) {
        const int32_t c = template_class ? template_class[k] : k;
        if (c < 0 || c >= n_classes) return fail(SYLDET_ERR_INVALID_ARGUMENT, "template " + std::to_string(k) + "'s class is outside [0, " + std::to_string(n_classes) + ")");
        members |= 1u << c;
    }
    if (members != (1u << n_classes) - 1u) return fail(SYLDET_ERR_INVALID_ARGUMENT, "a class has no template");
    sd::match_classes(template_scores, n_positions, n_templates, template_class, n_classes, class_scores, which);
    return SYLDET_OK;
}

int syldet_match_normalize_host(const float *templ, int32_t n, int32_t bins, float *t_hat)
{
    if (int st = template_args(templ, n, bins)) return st;
    if (!t_hat) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    std::vector<float> tmp((size_t)n * bins);               // (a refused template leaves t_hat as it was)
    if (int st = normalise(templ, n, bins, tmp.data())) return st;
    std::memcpy(t_hat, tmp.data(), tmp.size() * sizeof(float));
    return SYLDET_OK;
}

int syldet_match_scores_host(const float *t_hat, int32_t n, int32_t bins, const float *columns, int64_t n_frames, float *scores)
{
    if (int st = template_args(t_hat, n, bins)) return st;
    if (n_frames < 0 || (n_frames > 0 && (!columns || !scores))) return fail(SYLDET_ERR_INVALID_ARGUMENT, "a NULL array or a negative count");
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int64_t p = 0; p < n_frames; p++) {
        if (p + n > n_frames) {
            scores[p] = nan;
            continue;
        }
        const float *x = columns + p * bins;
        float dot = 0.0f, E = 0.0f;
        for (int j = 0; j < n; j++) {
            float e = 0.0f;
            for (int b = 0; b < bins; b++) {
                const float v = x[j * bins + b];
                e = std::fmaf(v, v, e);
                dot = std::fmaf(std::isfinite(v) ? v : 0.0f, t_hat[j * bins + b], dot);
            }
            E = E + e;
        }
        scores[p] = !std::isfinite(E) ? nan : E == 0.0f ? 0.0f : (dot + 0.0f) / std::sqrt(E);
    }
    return SYLDET_OK;
}

int syldet_match_peaks_host(const float *scores, int64_t n_positions, float threshold, int32_t separation, int64_t origin, int64_t hop, int32_t anchor,
                            int64_t *events, int64_t capacity, int64_t *count, float *event_scores)
{
    if (int st = peaks_args(threshold, separation, capacity)) return st;
    if (n_positions < 0 || !count || (n_positions > 0 && !scores) || (capacity > 0 && !events))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "a NULL array or a negative count");
    if (anchor < 0 || anchor >= SYLDET_MATCH_MAX_TEMPLATE || hop < 1 || hop >= ((int64_t)1 << 31) || origin < 0 || origin >= ((int64_t)1 << 32) ||
        n_positions >= ((int64_t)1 << 31))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "anchor outside [0, 32768), origin outside [0, 2^32), hop outside [1, 2^31) or 2^31 positions");
    const int S = separation, k = S ? sd::match_level(S) : 0;
    const int64_t L = n_positions + 2 * (int64_t)S;
    std::vector<uint32_t> cur, nxt;
    try {
        // the keys with S absent positions on either side, then the maxima of every window of 2^k positions, pass by pass as the kernel
        cur.assign((size_t)L, 0u);
        nxt.assign((size_t)L, 0u);
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    for (int64_t p = 0; p < n_positions; p++) cur[(size_t)(p + S)] = sd::match_key(scores[p]);
    const std::vector<uint32_t> keys(cur.begin() + S, cur.begin() + S + n_positions);
    for (int lev = 0; lev < k; lev++) {
        const int64_t h = (int64_t)1 << lev;
        for (int64_t i = 0; i < L; i++) nxt[(size_t)i] = std::max(cur[(size_t)i], i + h < L ? cur[(size_t)(i + h)] : 0u);
        cur.swap(nxt);
    }
    const uint32_t tk = sd::match_key(threshold);
    int64_t n = 0;
    for (int64_t p = 0; p < n_positions; p++) {
        const int64_t i = p + S;
        if (!sd::match_rule(keys[(size_t)p], sd::match_left(cur.data(), i, S, k), sd::match_right(cur.data(), i, S, k), tk)) continue;
        if (n < capacity) {
            events[n] = sd::match_event(origin, hop, p, anchor);
            if (event_scores) event_scores[n] = scores[p];
        }
        n++;
    }
    *count = n;
    return SYLDET_OK;
}

}  // extern "C"
