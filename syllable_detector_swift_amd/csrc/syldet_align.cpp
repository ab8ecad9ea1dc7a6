// syldet_align.cpp -- event-aligned windows (include/syldet.h, "event-aligned windows"; kernels_align.hip): the aligner that keeps a
// packed plan's detectors, the caller's event prefix and its group order on the device, so that syldet_align_device and
// syldet_align_stats_device are launches only; and the same text on the host (align_span.hpp, one detector; the block tree).

#include "align_span.hpp"
#include "syldet_handle.hpp"

static_assert(SYLDET_ALIGN_COLUMNS == sd::kAlignColumns && SYLDET_ALIGN_OUTPUTS == sd::kAlignOutputs && SYLDET_ALIGN_SAMPLES == sd::kAlignSamples,
              "the header's sources are the span's");
static_assert(SYLDET_ALIGN_MAX_WINDOW == sd::kAlignMaxWindow && SYLDET_ALIGN_BLOCK == sd::kAlignBlock, "the header's limits are the kernels'");

struct syldet_aligner : sd::DetectorTable {  // (the spans: units of the source)
    int source = 0, width = 0;
    int64_t before = 0, after = 0, origin = 0, step = 1;
    sd::DeviceBuffer d_dets;                 // (packed) the spans
    hipStream_t last = nullptr;              // the stream of the last call that may still read or write the tables below

    // the kept event prefix, and what is sized by it
    bool has_begin = false, has_spans = false;
    std::vector<int64_t> begin;              // [D + 1]
    sd::DeviceBuffer d_begin, d_spans;       // int64 [D + 1]; int2 [N]
    // the kept group order (of the kept prefix), and the partials
    bool has_groups = false;
    std::vector<int32_t> group;              // [D]
    int G = 0;
    sd::DeviceBuffer d_order, d_part;        // perm [N] | group_begin [G + 1] | block_begin [G + 1] | block_group [B]; count | sum | sumsq [B][L]
    sd::AlignStatsDesc stats{};

    int64_t N() const { return has_begin ? begin[(size_t)D] : 0; }
    int64_t L() const { return (before + after + 1) * width; }
};

namespace {

int window_args(int32_t source, int64_t before, int64_t after, int64_t width)
{
    if (source != SYLDET_ALIGN_COLUMNS && source != SYLDET_ALIGN_OUTPUTS && source != SYLDET_ALIGN_SAMPLES)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "source " + std::to_string(source) + " is none of SYLDET_ALIGN_COLUMNS, _OUTPUTS, _SAMPLES");
    if (before < 0 || after < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "before and after must not be negative");
    if (before > SYLDET_ALIGN_MAX_WINDOW || after > SYLDET_ALIGN_MAX_WINDOW || (before + after + 1) * width > SYLDET_ALIGN_MAX_WINDOW)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "a window of (before + after + 1) x width = " + std::to_string(before + after + 1) + " x " +
                                                     std::to_string(width) + " elements is above the limit of " + std::to_string(SYLDET_ALIGN_MAX_WINDOW));
    return SYLDET_OK;
}

// event_begin: D + 1 entries from 0 that do not decrease
int begin_args(const int64_t *event_begin, int D)
{
    if (!event_begin) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL event_begin");
    if (event_begin[0] != 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "event_begin[0] must be 0");
    for (int d = 0; d < D; d++)
        if (event_begin[d + 1] < event_begin[d]) return fail(SYLDET_ERR_INVALID_ARGUMENT, "event_begin[" + std::to_string(d + 1) + "] decreases");
    return SYLDET_OK;
}

// the anchor rule of a source on a bank
void anchor_of(const sd::BankInfo &b, int source, int64_t *origin, int64_t *step, int *width)
{
    if (source == SYLDET_ALIGN_COLUMNS) {
        *origin = (int64_t)b.geom.gap + b.window_length;
        *step = b.geom.hop;
        *width = b.geom.bins;
    } else if (source == SYLDET_ALIGN_OUTPUTS) {
        *origin = b.geom.first_index;
        *step = b.geom.hop;
        *width = b.geom.outputs;
    } else {
        *origin = 0;
        *step = 1;
        *width = 1;
    }
}

// One detector's windows in plain C++: the text the kernel's teams run, element by element.
void align_one(const float *src, int64_t U, int width, int64_t origin, int64_t step, int64_t before, int64_t after, const int64_t *events,
               int64_t n_events, float fill, float *windows, int64_t *present)
{
    const int64_t L = (before + after + 1) * width;
    for (int64_t j = 0; j < n_events; j++) {
        const sd::AlignSpan sp = sd::align_span(events[j], origin, step, before, after, U);
        const int64_t p0 = sp.first * width, p1 = p0 + sp.count * width;
        float *dst = windows + j * L;
        for (int64_t p = 0; p < p0; p++) dst[p] = fill;
        if (p1 > p0) std::memcpy(dst + p0, src + sp.unit * width, (size_t)(p1 - p0) * sizeof(float));
        for (int64_t p = p1; p < L; p++) dst[p] = fill;
        if (present) {
            present[2 * j] = p0;
            present[2 * j + 1] = p1 - p0;
        }
    }
}

}  // namespace

extern "C" {

int syldet_align_anchor(const syldet_t *h, int32_t source, int64_t *origin, int64_t *step, int32_t *width)
{
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (int st = window_args(source, 0, 0, 1)) return st;
    sd::BankInfo b{};
    sd::bank_info(h, &b);
    if (source == SYLDET_ALIGN_COLUMNS && h->classes.size() > 1)
        return fail(SYLDET_ERR_UNSUPPORTED, "columns of a mixed bank: its classes' columns are ragged");
    int64_t o = 0, s = 1;
    int w = 1;
    anchor_of(b, source, &o, &s, &w);
    if (origin) *origin = o;
    if (step) *step = s;
    if (width) *width = w;
    return SYLDET_OK;
}

int syldet_aligner_create(const syldet_t *h, const syldet_recordings_t *r, int32_t source, int64_t before, int64_t after, syldet_aligner_t **out)
{
    if (!out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (int st = window_args(source, before, after, 1)) return st;
    sd::BankInfo b{};
    sd::bank_info(h, &b);
    if (source == SYLDET_ALIGN_COLUMNS && h->classes.size() > 1)
        return fail(SYLDET_ERR_UNSUPPORTED, "columns of a mixed bank: its classes' columns are ragged");
    int64_t origin = 0, step = 1;
    int width = 1;
    anchor_of(b, source, &origin, &step, &width);
    if (int st = window_args(source, before, after, width)) return st;
    const sd::SpanUnit unit = source == SYLDET_ALIGN_COLUMNS ? sd::kSpanFrames : source == SYLDET_ALIGN_OUTPUTS ? sd::kSpanEvals : sd::kSpanSamples;

    std::unique_ptr<syldet_aligner, int (*)(syldet_aligner_t *)> a(nullptr, syldet_aligner_destroy);
    try {
        a.reset(new syldet_aligner());
        if (int st = a->read(h, r, unit)) return st;
        a->begin.assign((size_t)a->D + 1, 0);
        a->group.assign((size_t)a->D, 0);
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    a->source = source;
    a->width = width;
    a->before = before;
    a->after = after;
    a->origin = origin;
    a->step = step;
    if (!a->spans.empty()) {
        SYLDET_HIP(hipSetDevice(b.device));
        if (int st = a->d_dets.reserve(bytes_of(a->spans))) return st;
        SYLDET_HIP(upload(a->d_dets.ptr, 0, a->spans));
    }
    *out = a.release();
    return SYLDET_OK;
}

int syldet_aligner_destroy(syldet_aligner_t *a)
{
    if (!a) return SYLDET_OK;
    if (a->d_dets.ptr || a->d_begin.ptr || a->d_spans.ptr || a->d_order.ptr || a->d_part.ptr) (void)hipSetDevice(a->bank.device);
    a->d_dets.release();
    a->d_begin.release();
    a->d_spans.release();
    a->d_order.release();
    a->d_part.release();
    delete a;
    return SYLDET_OK;
}

int syldet_aligner_shape(const syldet_aligner_t *a, int32_t *n_detectors, int64_t *n_units_per_window, int32_t *width)
{
    if (!a) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_detectors) *n_detectors = a->D;
    if (n_units_per_window) *n_units_per_window = a->before + a->after + 1;
    if (width) *width = a->width;
    return SYLDET_OK;
}

int syldet_align_device(syldet_aligner_t *a, const float *d_src, int64_t n_units, int64_t row_stride, const int64_t *d_events,
                        int64_t event_stride, const int64_t *event_begin, float fill, float *d_windows, void *hip_stream)
{
    if (!a) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (int st = begin_args(event_begin, a->D)) return st;
    const int64_t N = event_begin[a->D], L = a->L();
    if (n_units < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_units is negative");
    if (N > 0 && ((n_units > 0 && !d_src) || !d_events || !d_windows)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int st = a->row_units_arg(n_units, "n_units", "units of this source")) return st;
    if (n_units > ((int64_t)1 << 40) / a->width) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_units x width is above 2^40");
    if (row_stride == 0) row_stride = n_units * a->width;
    if (row_stride < n_units * a->width)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "row_stride " + std::to_string(row_stride) + " is below the " + std::to_string(n_units * a->width) + " elements of a row");
    if (event_stride < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "event_stride is negative");
    if (event_stride > 0)
        for (int d = 0; d < a->D; d++)
            if (event_begin[d + 1] - event_begin[d] > event_stride)
                return fail(SYLDET_ERR_INVALID_ARGUMENT, "event_stride " + std::to_string(event_stride) + " is below the " +
                                                             std::to_string(event_begin[d + 1] - event_begin[d]) + " events of detector " + std::to_string(d));
    if (N > ((int64_t)1 << 40) / L) return fail(SYLDET_ERR_UNSUPPORTED, "more than 2^40 window elements");
    if (N > 0x7fffffff) return fail(SYLDET_ERR_UNSUPPORTED, "more than 2^31 - 1 windows");   // (a workgroup a window at the most: the grid)
    if (N == 0 && a->has_begin && a->N() == 0) return SYLDET_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    SYLDET_HIP(hipSetDevice(a->bank.device));
    if (!(a->has_begin && std::memcmp(a->begin.data(), event_begin, ((size_t)a->D + 1) * sizeof(int64_t)) == 0)) {
        // other arrays than the kept ones (the first call always): behind the last call, the tables sized by them and one blocking copy
        if (a->has_begin) SYLDET_HIP(hipStreamSynchronize(a->last));
        a->has_begin = a->has_spans = a->has_groups = false;
        if (int st = a->d_begin.reserve(((size_t)a->D + 1) * sizeof(int64_t))) return st;
        if (int st = a->d_spans.reserve((size_t)std::max<int64_t>(N, 1) * sizeof(int2))) return st;
        SYLDET_HIP(hipMemcpy(a->d_begin.ptr, event_begin, ((size_t)a->D + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        std::memcpy(a->begin.data(), event_begin, ((size_t)a->D + 1) * sizeof(int64_t));
        a->has_begin = true;
    }
    a->last = stream;
    if (N == 0) return SYLDET_OK;
    sd::AlignDesc desc{};
    desc.dets = a->packed ? (const sd::DetSpan *)a->d_dets.ptr : nullptr;
    desc.event_begin = (const int64_t *)a->d_begin.ptr;
    desc.spans = (int2 *)a->d_spans.ptr;
    desc.D = a->D;
    desc.width = a->width;
    desc.origin = a->origin;
    desc.step = a->step;
    desc.before = a->before;
    desc.after = a->after;
    a->h->prof_begin();
    KernelTimer t(a->h, stream, "align_windows_kernel");
    SYLDET_HIP(sd::launch_align_windows(desc, d_src, n_units, row_stride, d_events, event_stride, N, fill, d_windows, stream));
    a->has_spans = true;
    return SYLDET_OK;
}

int syldet_align_stats_device(syldet_aligner_t *a, const float *d_windows, const int64_t *event_begin, const int32_t *group, int32_t n_groups,
                              int64_t *d_count, double *d_sum, double *d_sumsq, void *hip_stream)
{
    if (!a) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (int st = begin_args(event_begin, a->D)) return st;
    if (n_groups < 1) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_groups must be at least 1");
    if (!d_count || !d_sum || !d_sumsq || (a->D > 0 && !group)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    for (int d = 0; d < a->D; d++)
        if (group[d] < 0 || group[d] >= n_groups)
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "group[" + std::to_string(d) + "] = " + std::to_string(group[d]) + " is outside [0, " + std::to_string(n_groups) + ")");
    const int64_t N = event_begin[a->D], L = a->L();
    if (N > 0 && !d_windows) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!a->has_begin || std::memcmp(a->begin.data(), event_begin, ((size_t)a->D + 1) * sizeof(int64_t)) != 0 || (N > 0 && !a->has_spans))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "event_begin is not that of the aligner's last syldet_align_device call, whose windows the statistics describe");
    const int chunks = (int)((L + 255) / 256);
    if ((N / SYLDET_ALIGN_BLOCK + n_groups) * chunks > 0x7fffffff) return fail(SYLDET_ERR_UNSUPPORTED, "more than 2^31 - 1 workgroups");
    hipStream_t stream = (hipStream_t)hip_stream;
    SYLDET_HIP(hipSetDevice(a->bank.device));
    if (!(a->has_groups && a->G == n_groups && (a->D == 0 || std::memcmp(a->group.data(), group, (size_t)a->D * sizeof(int32_t)) == 0))) {
        SYLDET_HIP(hipStreamSynchronize(a->last));
        a->has_groups = false;
        std::vector<int64_t> host;
        int64_t B = 0;
        const size_t G = (size_t)n_groups;
        try {
            // the group order: detector ascending, then event ascending (a counting sort by group keeps both)
            std::vector<int64_t> gb(G + 1, 0), bb(G + 1, 0);
            for (int d = 0; d < a->D; d++) gb[(size_t)group[d] + 1] += event_begin[d + 1] - event_begin[d];
            for (size_t g = 0; g < G; g++) {
                bb[g + 1] = bb[g] + (gb[g + 1] + SYLDET_ALIGN_BLOCK - 1) / SYLDET_ALIGN_BLOCK;
                gb[g + 1] += gb[g];
            }
            B = bb[G];
            // perm [N] | group_begin [G + 1] | block_begin [G + 1] | block_group [B] (int32, two a word)
            host.assign((size_t)N + 2 * (G + 1) + (size_t)(B + 1) / 2, 0);
            std::vector<int64_t> at(gb.begin(), gb.end() - 1);
            for (int d = 0; d < a->D; d++)
                for (int64_t w = event_begin[d]; w < event_begin[d + 1]; w++) host[(size_t)at[(size_t)group[d]]++] = w;
            std::memcpy(host.data() + N, gb.data(), (G + 1) * sizeof(int64_t));
            std::memcpy(host.data() + N + (int64_t)G + 1, bb.data(), (G + 1) * sizeof(int64_t));
            int32_t *bg = (int32_t *)(host.data() + N + 2 * ((int64_t)G + 1));
            for (size_t g = 0; g < G; g++)
                for (int64_t blk = bb[g]; blk < bb[g + 1]; blk++) bg[blk] = (int32_t)g;
        } catch (const std::bad_alloc &) {
            return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
        }
        if (int st = a->d_order.reserve(host.size() * sizeof(int64_t) + 8)) return st;
        if (int st = a->d_part.reserve((size_t)std::max<int64_t>(B, 1) * (size_t)L * 24)) return st;
        SYLDET_HIP(hipMemcpy(a->d_order.ptr, host.data(), host.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        int64_t *base = (int64_t *)a->d_order.ptr;
        a->stats.perm = base;
        a->stats.group_begin = base + N;
        a->stats.block_begin = base + N + n_groups + 1;
        a->stats.block_group = (const int32_t *)(base + N + 2 * ((int64_t)n_groups + 1));
        a->stats.part_count = (int64_t *)a->d_part.ptr;
        a->stats.part_sum = (double *)a->d_part.ptr + B * L;
        a->stats.part_sumsq = (double *)a->d_part.ptr + 2 * B * L;
        a->stats.G = n_groups;
        a->stats.B = B;
        if (a->D > 0) std::memcpy(a->group.data(), group, (size_t)a->D * sizeof(int32_t));
        a->G = n_groups;
        a->has_groups = true;
    }
    a->stats.spans = (const int2 *)a->d_spans.ptr;
    a->last = stream;
    a->h->prof_begin();
    {
        KernelTimer t(a->h, stream, "align_stats_kernel");
        SYLDET_HIP(sd::launch_align_stats(a->stats, d_windows, (int)L, stream));
    }
    KernelTimer t(a->h, stream, "align_combine_kernel");
    SYLDET_HIP(sd::launch_align_combine(a->stats, (int)L, d_count, d_sum, d_sumsq, stream));
    return SYLDET_OK;
}

int syldet_align_host(const float *src, int64_t n_units, int32_t width, int64_t origin, int64_t step, int64_t before, int64_t after,
                      const int64_t *events, int64_t n_events, float fill, float *windows, int64_t *present)
{
    if (width < 1 || width > SYLDET_ALIGN_MAX_WINDOW) return fail(SYLDET_ERR_INVALID_ARGUMENT, "width must be in [1, 2^20]");
    if (int st = window_args(SYLDET_ALIGN_SAMPLES, before, after, width)) return st;
    if (n_units < 0 || n_units >= sd::kAlignEventLimit / width || n_events < 0 || (n_units > 0 && !src) || (n_events > 0 && (!events || !windows)))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "a NULL array or a count out of range");
    if (origin < 0 || origin >= ((int64_t)1 << 32) || step < 1 || step >= ((int64_t)1 << 31))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "origin outside [0, 2^32) or step outside [1, 2^31)");
    align_one(src, n_units, width, origin, step, before, after, events, n_events, fill, windows, present);
    return SYLDET_OK;
}

int syldet_align_stats_host(const float *windows, const int64_t *present, int64_t n_events, int64_t window_elements, int64_t *count,
                            double *sum, double *sumsq)
{
    if (n_events < 0 || window_elements < 1 || window_elements > SYLDET_ALIGN_MAX_WINDOW || !count || !sum || !sumsq ||
        (n_events > 0 && (!windows || !present)))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "a NULL array, a negative count or a window above the limit");
    const int64_t L = window_elements;
    for (int64_t i = 0; i < n_events; i++)
        if (present[2 * i] < 0 || present[2 * i + 1] < 0 || present[2 * i] + present[2 * i + 1] > L)
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "present[" + std::to_string(i) + "] reaches outside the window");
    for (int64_t p = 0; p < L; p++) {
        int64_t n = 0;
        double s = 0.0, q = 0.0;
        for (int64_t i0 = 0; i0 < n_events; i0 += SYLDET_ALIGN_BLOCK) {
            double bs = 0.0, bq = 0.0;
            const int64_t i1 = std::min<int64_t>(i0 + SYLDET_ALIGN_BLOCK, n_events);
            for (int64_t i = i0; i < i1; i++) {
                if (p < present[2 * i] || p >= present[2 * i] + present[2 * i + 1]) continue;
                const double x = (double)windows[i * L + p];
                n++;
                bs = bs + x;
                bq = bq + x * x;                                          // (exact: the square of an fp32 value has 48 bits)
            }
            s = s + bs;
            q = q + bq;
        }
        count[p] = n;
        sum[p] = s;
        sumsq[p] = q;
    }
    return SYLDET_OK;
}

}  // extern "C"
