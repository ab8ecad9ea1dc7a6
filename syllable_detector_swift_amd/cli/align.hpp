// --align-dir: the run's state, the windows of one bank's events, one file's files and the stacks over all files (see AlignOpt).
#pragma once

#include <hip/hip_runtime.h>

#include "score.hpp"

namespace {

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1) == hipSuccess; }
};

struct AlignRun {
    AlignOpt opt;
    const Labels *labels = nullptr;                        // --align-at labels: --score's file
    int64_t before = 0, after = 0, n = 0;
    int width = 1, networks = 1;
    struct Stack {
        std::vector<int64_t> count;
        std::vector<double> sum, sumsq;
        std::vector<float> block;                          // the windows of the block being gathered
        std::vector<int64_t> present;
        int64_t held = 0;
    };
    std::vector<Stack> stacks;
    bool failed = false;
    int64_t L() const { return n * width; }
};

// One bank's events and windows: detector d -- a batch's recording, or a file's track -- has events[d], units[d] units of the source
// (what decides which elements of a window are present) and its windows from begin[d]
struct Aligned {
    std::vector<std::vector<int64_t>> events;
    std::vector<int64_t> units, begin;
    std::vector<float> windows;
    int64_t origin = 0, step = 1;
    bool made = false;
};

// What a bank holds on the device that windows can be cut from, and every detector's share of it
struct AlignInput {
    const float *rows;                                      // the fp32 rows the detector was fed, row_samples each, stride apart
    int64_t row_samples, stride;
    int64_t samples_stride;                                 // ... as syldet_align_device is told for the samples (0: packed rows)
    const float *out;                                       // the outputs the run left, row_evals a row
    int64_t row_evals;
    int C;
    std::vector<int64_t> samples, evals;                    // what each detector has
    hipStream_t stream;
};

// ... and the choice --align makes: the array, its units a row, the rows' distance; st: what the library said on the way
struct AlignSource {
    const float *src = nullptr;
    int64_t n_units = 0, row_stride = 0;
    int st = 0;
};

// The window's size from the options and the networks, the empty stacks, the directory.  0, or the usage error.
int align_begin(AlignRun &run, const AlignOpt &opt, const std::vector<syldet_config_t *> &cfgs, const Labels *labels)
{
    syldet_geometry_t g;
    const int gst = syldet_config_geometry(cfgs[0], &g);
    run.opt = opt;
    run.labels = labels;
    run.before = opt.before < 0 ? cfgs[0]->time_range - 1 : opt.before;
    run.after = opt.after < 0 ? cfgs[0]->time_range - 1 : opt.after;
    run.n = run.before + run.after + 1;
    run.width = opt.source == SYLDET_ALIGN_COLUMNS ? g.bins : opt.source == SYLDET_ALIGN_OUTPUTS ? cfgs[0]->n_thresholds : 1;
    run.networks = (int)cfgs.size();
    if (gst) return fail(std::string("Unable to use the network configuration: ") + syldet_strerror(gst) + ": " + syldet_last_error());
    if (run.width < 1 || run.L() > SYLDET_ALIGN_MAX_WINDOW) return fail("--align-before and --align-after: a window may hold " + std::to_string(SYLDET_ALIGN_MAX_WINDOW) + " values at most.");
    run.stacks.resize(cfgs.size());
    for (AlignRun::Stack &st : run.stacks) {
        st.count.assign((size_t)run.L(), 0);
        st.sum.assign((size_t)run.L(), 0.0);
        st.sumsq.assign((size_t)run.L(), 0.0);
    }
    std::error_code ec;
    std::filesystem::create_directories(opt.dir, ec);
    return 0;
}

// the events --align-at names for one track of one file: its labels (--score's file), or the detections given
std::vector<int64_t> align_events_of(const AlignRun &run, const std::string &path, int track, const int64_t *detections, int64_t n)
{
    if (!run.opt.at_labels) return std::vector<int64_t>(detections, detections + n);
    return labels_of(*run.labels, path, track);
}

// The source --align names, of the arrays a bank holds: the outputs the run left, the fp32 rows, or their columns
// (syldet_spectrogram_device into d_cols), and the units every detector has of it.  s.st on entry: skip the launch.  false: no memory.
bool align_source(const AlignRun &run, syldet_t *h, const AlignInput &in, DevBuf &d_cols, AlignSource &s, std::vector<int64_t> &units)
{
    const int64_t J = std::max<int64_t>(0, syldet_count_frames(h, in.row_samples));
    units.assign(in.samples.size(), 0);
    if (run.opt.source == SYLDET_ALIGN_SAMPLES) {
        s.src = in.rows;
        s.n_units = in.row_samples;
        s.row_stride = in.samples_stride;
        units = in.samples;
    } else if (run.opt.source == SYLDET_ALIGN_COLUMNS) {
        if (!d_cols.alloc((size_t)in.C * (size_t)J * (size_t)run.width * sizeof(float))) return false;
        if (!s.st && J > 0) s.st = syldet_spectrogram_device(h, in.rows, in.row_samples, in.stride, (float *)d_cols.p, in.stream);
        s.src = (const float *)d_cols.p;
        s.n_units = J;
        for (size_t i = 0; i < units.size(); i++) units[i] = std::max<int64_t>(0, syldet_count_frames(h, in.samples[i]));
    } else {
        s.src = in.out;
        s.n_units = in.row_evals;
        units = in.evals;
    }
    return true;
}

// The windows of one bank's detectors -- a batch's recordings (r), or a file's tracks (r NULL) -- in one launch, and back: windows
// [N][n][width] with detector d's events from begin[d].  s.src: the source on the device, s.n_units units a row.
bool align_windows(AlignRun &run, syldet_t *h, syldet_recordings_t *r, const AlignSource &s, hipStream_t stream, Aligned &al)
{
    al.begin.assign(1, 0);
    std::vector<int64_t> flat;
    for (const std::vector<int64_t> &e : al.events) {
        flat.insert(flat.end(), e.begin(), e.end());
        al.begin.push_back((int64_t)flat.size());
    }
    const int64_t N = al.begin.back();
    al.windows.assign((size_t)N * (size_t)run.L(), 0.0f);
    syldet_aligner_t *a = nullptr;
    int st = syldet_aligner_create(h, r, run.opt.source, run.before, run.after, &a);
    DevBuf d_events, d_windows;
    bool ok = true;
    if (!st && N > 0) {
        ok = d_events.alloc(flat.size() * sizeof(int64_t)) && d_windows.alloc(al.windows.size() * sizeof(float)) &&
             hipMemcpyAsync(d_events.p, flat.data(), flat.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream) == hipSuccess;
        if (ok) st = syldet_align_device(a, s.src, s.n_units, s.row_stride, (const int64_t *)d_events.p, 0, al.begin.data(), std::nanf(""), (float *)d_windows.p, stream);
        if (ok && !st) ok = hipMemcpyAsync(al.windows.data(), d_windows.p, al.windows.size() * sizeof(float), hipMemcpyDeviceToHost, stream) == hipSuccess;
    }
    if (ok && hipStreamSynchronize(stream) != hipSuccess) ok = false;
    syldet_aligner_destroy(a);
    if (st) std::fprintf(stderr, "Unable to align the events: %s: %s\n", syldet_strerror(st), syldet_last_error());
    return ok && st == 0;
}

// one block of a stack into its totals: the block alone through the library's tree (one block: its own sums), then total + block
void align_flush(AlignRun &run, AlignRun::Stack &st)
{
    if (st.held == 0) return;
    const size_t L = (size_t)run.L();
    std::vector<int64_t> c(L);
    std::vector<double> s(L), q(L);
    if (syldet_align_stats_host(st.block.data(), st.present.data(), st.held, (int64_t)L, c.data(), s.data(), q.data())) {
        std::fprintf(stderr, "Unable to add the aligned windows: %s: %s\n", syldet_strerror(SYLDET_ERR_INVALID_ARGUMENT), syldet_last_error());
        run.failed = true;
    }
    for (size_t p = 0; p < L; p++) {
        st.count[p] += c[p];
        st.sum[p] = st.sum[p] + s[p];
        st.sumsq[p] = st.sumsq[p] + q[p];
    }
    st.held = 0;
}

// One audio file's windows and their table, and its events into the networks' stacks: track by track, event by event.  The file's
// tracks are the bank's detectors k0 .. k0 + tracks - 1.  0, or 3: a file is not written.
int align_write_file(AlignRun &run, const std::string &path, const Aligned &al, size_t k0, int tracks, double rate)
{
    if (!al.made) return 3;
    const int64_t L = run.L();
    const float *windows = al.windows.data() + (size_t)al.begin[k0] * (size_t)L;
    const int64_t N = al.begin[k0 + (size_t)tracks] - al.begin[k0];
    const std::string npy = TrackDirs::in(run.opt.dir, path, ".npy"), tsv = TrackDirs::in(run.opt.dir, path, ".tsv");
    int bad = 0;
    if (!write_npy(npy, "<f4", {N, run.n, (int64_t)run.width}, windows, (size_t)N * (size_t)L * sizeof(float))) bad = 3;
    FILE *f = std::fopen(tsv.c_str(), "w");
    bool ok = f != nullptr;
    int64_t w = 0;
    for (size_t t = 0; t < (size_t)tracks; t++) {
        AlignRun::Stack &st = run.stacks[run.networks > 1 ? t % (size_t)run.networks : 0];
        for (const int64_t s : al.events[k0 + t]) {
            if (ok) ok = std::fputs((std::to_string(t) + "\t" + std::to_string(s) + "\t" + number((double)s / rate) + "\n").c_str(), f) >= 0;
            // the present elements of the window: the units u0 - before .. u0 + after that lie in [0, units) (include/syldet.h)
            const int64_t c = s < -(((int64_t)1 << 62) - 1) ? -(((int64_t)1 << 62) - 1) : s > ((int64_t)1 << 62) - 1 ? ((int64_t)1 << 62) - 1 : s;
            int64_t u0 = (c - al.origin) / al.step;
            if (u0 * al.step > c - al.origin) u0--;          // a floor, also for a negative numerator
            const int64_t lo = u0 - run.before, first = std::max<int64_t>(lo, 0), last = std::min<int64_t>(u0 + run.after, al.units[k0 + t] - 1);
            st.block.insert(st.block.end(), windows + w * L, windows + (w + 1) * L);
            st.present.push_back(last >= first ? (first - lo) * run.width : 0);
            st.present.push_back(last >= first ? (last - first + 1) * run.width : 0);
            w++;
            if (++st.held == SYLDET_ALIGN_BLOCK) {
                align_flush(run, st);
                st.block.clear();
                st.present.clear();
            }
        }
    }
    if (f && std::fclose(f) != 0) ok = false;
    if (!ok) {
        std::fprintf(stderr, "Unable to write %s.\n", tsv.c_str());
        bad = 3;
    }
    return bad;
}

// the three stack files, behind the last audio file
bool align_finish(AlignRun &run)
{
    const size_t L = (size_t)run.L();
    std::vector<int64_t> count;
    std::vector<double> sum, sumsq;
    for (AlignRun::Stack &st : run.stacks) {
        align_flush(run, st);
        count.insert(count.end(), st.count.begin(), st.count.end());
        sum.insert(sum.end(), st.sum.begin(), st.sum.end());
        sumsq.insert(sumsq.end(), st.sumsq.begin(), st.sumsq.end());
    }
    const std::vector<int64_t> shape = {(int64_t)run.networks, run.n, (int64_t)run.width};
    bool ok = !run.failed;
    for (int i = 0; i < 3; i++) {
        const std::string path = run.opt.dir + (i == 0 ? "/count.npy" : i == 1 ? "/sum.npy" : "/sumsq.npy");
        const void *data = i == 0 ? (const void *)count.data() : i == 1 ? (const void *)sum.data() : (const void *)sumsq.data();
        if (!write_npy(path, i == 0 ? "<i8" : "<f8", shape, data, L * run.stacks.size() * 8)) ok = false;
    }
    return ok;
}

}  // namespace
