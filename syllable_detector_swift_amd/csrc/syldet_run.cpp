// syldet_run.cpp -- the batch calls: which kernels run a batch and their dispatch on a stream, the host-pointer pipeline, the
// interleaved forms, spectrogram and detections, and the dry-run seam behind syldet_fused_form_of_config.

#include "syldet_handle.hpp"

namespace {

// The calling thread's most recent batch call: the handle it went through and, if a fused kernel ran, the instantiation its
// launcher recorded (kernels.hpp, FusedForm) -- syldet_last_fused_form.  A class handle's launch counts for its bank.
struct LastCall {
    const syldet *h = nullptr;
    bool fused = false;
    FusedForm form{};
};
thread_local LastCall t_last_call;
void note_call(const syldet *h, bool fused)        // a batch call begins (false); a fused launcher has just run for it (true)
{
    t_last_call = LastCall{h->root ? h->root : h, fused, fused ? fused_seam().last : FusedForm{}};
}

// The exact recomputation behind a fused kernel: on ordinary audio an empty launch behind EVERY batch call, so it gets no events of
// its own (two event records are ~9 us on the stream: 1 % of the headline's step) -- it times itself (the device's 100 MHz counter,
// first workgroup in to last workgroup out) and leaves its work list's length and its duration in two page-locked words of the
// call's slot; syldet_timings lists it for the calls that gave it work (a loud recording through a network without a normaliser can
// spend ten times the fused kernel's time here: MEASUREMENTS R5.7).
template <class F>
int timed_fixup(syldet *hc, hipStream_t stream, FixList list, F launch)
{
    syldet *h = hc->root ? hc->root : hc;             // (a class handle: its bank's profile)
    if (h->profiling && !h->prof_calls.empty() && list.counters) {
        if (h->prof_items_n < h->prof_depth) {
            // (the first profiled call since the history's depth grew: once, and nothing may still be writing the old array)
            SYLDET_HIP(hipDeviceSynchronize());
            if (h->prof_items) (void)hipHostFree(h->prof_items);
            h->prof_items = nullptr; h->prof_items_dev = nullptr; h->prof_items_n = 0;
            SYLDET_HIP(hipHostMalloc(reinterpret_cast<void **>(&h->prof_items), 2 * sizeof(unsigned) * (size_t)h->prof_depth, hipHostMallocMapped));
            SYLDET_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&h->prof_items_dev), h->prof_items, 0));
            h->prof_items_n = h->prof_depth;
            for (int i = 0; i < 2 * h->prof_items_n; i++) h->prof_items[i] = 0u;
        }
        syldet::ProfCall &pc = h->prof_calls[(size_t)h->prof_cur()];
        pc.fix = true;
        pc.fix_stream = stream;
        list.host_count = h->prof_items_dev + 2 * h->prof_cur();
    }
    SYLDET_HIP(launch(list));
    return SYLDET_OK;
}

// The work list for one launch over `units` evaluations (or frames) per channel: room for every 16-unit tile of every
// segment of every channel, so the list cannot overflow; the counters are zeroed when the buffer is (re)allocated and by the
// recomputation kernel itself after every launch.  SYLDET_NO_GUARD=1 (diagnostic A/B only) turns the guard off.
int prepare_fix(syldet *h, int C, int64_t units, int64_t segments, hipStream_t stream, FixList &out)
{
    out = FixList{nullptr, nullptr, 0};
    if (!h->has_fix || h->sw.no_guard) return SYLDET_OK;
    // (a list for every tile of every segment cannot overflow; past 2^26 items -- a gigabyte of list, batches of 10^9
    // evaluations -- it is bounded instead, and a kernel that finds it full raises the sticky overflow flag that
    // syldet_fixup_stats reports: the guard is never silently off)
    uint64_t cap = (uint64_t)C * (uint64_t)((units + 15) / 16 + 8 * segments + 16);
    if (cap > (1ull << 26)) cap = 1ull << 26;
    const size_t bytes = 32 + (size_t)cap * sizeof(FixItem);
    if (bytes > h->d_fix.cap) {
        if (int st = h->d_fix.reserve(bytes + bytes / 4)) return st;
        SYLDET_HIP(hipMemsetAsync(h->d_fix.ptr, 0, 32, stream));
    }
    out.counters = (unsigned *)h->d_fix.ptr;
    out.items = (FixItem *)((char *)h->d_fix.ptr + 32);
    out.capacity = (unsigned)cap;
    return SYLDET_OK;
}

// samples -> [C][J][F] columns: the fused engine's DFT half where its shape allows (and the handle was not created
// for the generic engine outright), the generic FFT otherwise
// row_of: a mixed bank's class launch, channel c reads bank row row_of[c] (the generic FFT kernels only)
// The transform's decision for J frames of C rows: whether a fused kernel's spectrogram instantiation takes them, the plan `d` it
// runs, and whether that is the fold kernel's (`fold`) or the 8-wave kernel's.  (stft_on_stream, syldet_fused_form_of_config)
bool dft_route_for(const syldet *h, int64_t J, int C, bool for_network, const int *row_of, float *d_columns, FusedDesc &d, bool &fold)
{
    // columns that go through log / dB keep the generic FFT: its error is relative to the frame, the block-floating-point
    // DFT's to the loudest sample of the 128-frame pass, and the logarithm turns relative error of weak bins into absolute
    const bool log_input = for_network && h->cfg.view.scaling != SYLDET_SCALING_LINEAR;
    // ... and columns that meet a network without a normaliser in front keep it too (normalised_chain above); the wide engine
    // is bf16 behind either
    const bool level_input = for_network && !normalised_chain(h->cfg.view) && h->engine != SYLDET_ENGINE_WIDE_BF16 && h->engine_asked == SYLDET_ENGINE_AUTO;
    if (!(h->has_dft && !log_input && !level_input && !row_of && (uint64_t)J * (uint64_t)h->geom.bins * 4u < 0xFFFFFFF0ull)) return false;
    d = h->dft.desc;
    fused_segmentation(d, J, C);
    d.spect_out = d_columns;
    apply_switches(h->sw, d);
    d.ko = 0;                                      // (the transform never takes the knock-out build)
    // the fold kernel's spectrogram instantiation where the plan allows it (rows under 2 GiB: its 32-bit byte offsets)
    fold = !h->sw.fused_nofold && fused_s_spectrogram_applicable(d) && ((J - 1) * (int64_t)d.hop + d.gap + d.W) * 4 < 0x7fffffffll;
    return fold || d.classic_ok;
}

int stft_on_stream(syldet *h, const float *d_samples, int64_t stride, int C, int64_t J, float *d_columns, hipStream_t stream,
                   bool for_network = true, const int *row_of = nullptr)
{
    FusedDesc d{};
    bool fold = false;
    if (dft_route_for(h, J, C, for_network, row_of, d_columns, d, fold)) {
        // the precision guard's work list, and behind the kernel the exact recomputation of the frames it reports
        if (int st = prepare_fix(h, C, J, (J + d.seg_evals - 1) / d.seg_evals + (d.s_seg_evals > 0 ? (J + d.s_seg_evals - 1) / d.s_seg_evals : 0), stream, d.fix)) return st;
        if (fold) {
            KernelTimer t(h, stream, "fused_s_kernel (spectrogram)");
            SYLDET_HIP(launch_fused_s_spectrogram(d, d_samples, stride, C, J, stream));
        } else {
            KernelTimer t(h, stream, "fused_kernel (spectrogram)");
            SYLDET_HIP(launch_fused_spectrogram(d, d_samples, stride, C, J, stream));
        }
        note_call(h, true);
        return timed_fixup(h, stream, d.fix, [&](const FixList &l) { return launch_fixup(h->fixd, h->net, d_samples, stride, J, 0, nullptr, nullptr, d_columns, l, stream); });
    }
    StftDesc sd = h->stft;
    sd.row_of = row_of;
    if (!h->sw.no_stft_lanes && stft_lanes_applicable(sd, d_samples, stride)) {
        KernelTimer t(h, stream, "stft_lanes_kernel");
        SYLDET_HIP(launch_stft_lanes(sd, d_samples, stride, C, J, d_columns, stream));
        return SYLDET_OK;
    }
    KernelTimer t(h, stream, "stft_generic_kernel");
    SYLDET_HIP(launch_stft_generic(sd, d_samples, stride, C, J, d_columns, stream));
    return SYLDET_OK;
}

// Which kernels run a batch: decided once per handle and batch (route_for); the widening of 16-bit rows, the timers' names and the
// launch (run_route) all read this one answer, and so does syldet_fused_form_of_config.
struct Route {
    // kNone: no evaluation in the batch; kMixed: each class has a route of its own; kColumns: stft_on_stream, then the matrix-core or the interpretive network stage
    enum Family { kNone, kMixed, kFused, kWide, kBdft, kFft1k, kColumns } family = kNone;
    int64_t J = 0, E = 0;       // the batch's frames and evaluations
    FusedDesc d{};              // kFused: the plan as it is launched (segmented for the batch, the handle's switches applied)
    int choice = 0;             // kFused: fused_choice(d, J) -- 0 the 8-wave kernel, 1 the register-resident-basis kernel, 2 the fold kernel
    bool native_s16 = false;    // kFused: 16-bit PCM rows are read as they are (the fold kernel's s16 form); every other route widens them first
};

// The route of S samples a row on C rows `stride` apart, 16-bit PCM or fp32, the first row at address `base`.
Route route_for(const syldet *h, int64_t S, int64_t stride, int C, bool s16, uintptr_t base)
{
    Route r;
    const int64_t J = r.J = count_frames(h, S), E = r.E = count_evals(h, S);
    if (E <= 0) return r;
    if (!h->classes.empty()) { r.family = Route::kMixed; return r; }
    // the fused kernel addresses a channel's results with 32-bit byte offsets; longer rows take the generic engine
    if (h->engine == SYLDET_ENGINE_FUSED && (uint64_t)E * (uint64_t)h->geom.outputs * 4u < 0xFFFFFFF0ull) {
        FusedDesc &d = r.d;
        d = h->fused.desc;
        fused_segmentation(d, E, C);
        d.fix = FixList{nullptr, nullptr, 0};
        apply_switches(h->sw, d);
        // Which fused kernel THIS batch gets is known only now (the fold kernel addresses a row with 32-bit byte offsets; a
        // diagnostic switch may rule it out).  The batch takes the fused route only if that kernel can run it (plans whose hop
        // only the fold kernel holds have no 8-wave form: classic_ok == 0) and, for log / dB columns under AUTO, only on the fold
        // kernel -- the one AUTO committed to for them at create time: the pass-scaled kernels do not hold 1e-5 there.  Anything
        // else goes to the generic engine below, like the long rows.
        const int choice = r.choice = fused_choice(d, J);
        const bool runnable = choice != 0 || d.classic_ok;
        const bool in_contract = ((h->cfg.view.scaling == SYLDET_SCALING_LINEAR && normalised_chain(h->cfg.view)) || choice == 2 || h->engine_asked == SYLDET_ENGINE_FUSED);
        bool fused_route = runnable && in_contract;
        // (a multi-network handle: only the fold kernel has the form; the diagnostic stamped builds are not for it)
        if ((h->n_nets > 1 || h->fnets) && (choice != 2 || h->sw.fused_stamps)) fused_route = false;
        if (fused_route) {
            r.family = Route::kFused;
            // 16-bit PCM on a kernel that reads int16 natively: the launcher's choice of the fold kernel's form (fused_s_native_s16),
            // and rows of whole 4-byte words (the DMA's) -- a 4-byte aligned base, an even stride and gap
            r.native_s16 = s16 && choice == 2 && !h->sw.fused_stamps && fused_s_native_s16(d) && (base & 3) == 0 && (stride & 1) == 0 && (d.gap & 1) == 0;
            return r;
        }
    }
    const float *rows = reinterpret_cast<const float *>(base);
    // (16-bit rows are widened first: the engines read widen_s16's copy -- a device allocation of its own, rows of whole quads)
    if (s16) { rows = nullptr; stride = (S + 3) & ~(int64_t)3; }
    if (h->engine == SYLDET_ENGINE_WIDE_BF16) r.family = Route::kWide;
    // frames of four hops: every block transformed once on the matrix cores, then the same network stage -- one launch
    else if (h->bdft.ok && !h->sw.no_bdft && (uint64_t)E * 4u < 0xFFFFFFF0ull && (uint64_t)S * 4u < 0x7fffffffull) r.family = Route::kBdft;
    // 1024-point frames in front of a network of the matrix-core class: one launch, the columns never leave the CU
    else if (h->mlpx.ok && !h->sw.no_fft1k && (uint64_t)E * 4u < 0xFFFFFFF0ull && fft1k_applicable(h->stft, h->mlpx.desc, rows, stride)) r.family = Route::kFft1k;
    else r.family = Route::kColumns;
    return r;
}

// 16-bit PCM rows for kernels that read fp32: one packed copy x * 2^-15 in the bank's scratch (d_widen; rows of whole 16-byte
// quads).  The conversion is exact and no engine's arithmetic depends on a row's alignment or stride (only its load widths do),
// so the batch gives the bits of the fp32 call on the same samples.  x and stride become the copy's.
int widen_s16(syldet *h, Samples &x, int64_t S, int64_t &stride, int C, hipStream_t stream)
{
    syldet *owner = h->root ? h->root : h;
    const int64_t ws = (S + 3) & ~(int64_t)3;
    if (int st = owner->d_widen.reserve((size_t)C * (size_t)ws * sizeof(float))) return st;
    {
        KernelTimer t(h, stream, "widen_s16_kernel");
        SYLDET_HIP(launch_widen_s16((const int16_t *)x.p, stride, S, C, (float *)owner->d_widen.ptr, ws, stream));
    }
    x = Samples((const float *)owner->d_widen.ptr);
    stride = ws;
    return SYLDET_OK;
}

int check_batch_args(const syldet *h, const void *samples, int64_t S, int64_t stride)
{
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (S < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_samples must be >= 0");
    if (!samples && S > 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL samples");
    // the stride only matters between rows; a single channel may pass anything
    if (h->channels > 1 && stride < S) return fail(SYLDET_ERR_INVALID_ARGUMENT, "channel_stride must be >= n_samples");
    return SYLDET_OK;
}

// diagnostic only: SYLDET_FUSED_STAMPS=1 runs the stamped instantiation of the fused route's kernel (`choice`) and prints where a
// workgroup pass spends its cycles (never set in tests or the benchmark)
int run_stamped(syldet *h, FusedDesc &d, int choice, const float *d_samples, int64_t stride, int C, int64_t S, int64_t J, int64_t E,
                float *d_outputs, uint8_t *d_flags, hipStream_t stream)
{
    // the stamped launch, and its n words on the host
    std::vector<unsigned long long> host;
    auto launch = [&](size_t n, const char *name) -> int {
        if (int st = h->d_stamps.reserve(n * sizeof(unsigned long long))) return st;
        SYLDET_HIP(hipMemsetAsync(h->d_stamps.ptr, 0, n * sizeof(unsigned long long), stream));
        d.stamps = (unsigned long long *)h->d_stamps.ptr;
        {
            KernelTimer t(h, stream, name);
            SYLDET_HIP(launch_fused(d, d_samples, stride, C, S, J, E, d_outputs, d_flags, stream));
        }
        host.resize(n);
        SYLDET_HIP(hipMemcpyAsync(host.data(), h->d_stamps.ptr, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        SYLDET_HIP(hipStreamSynchronize(stream));
        return SYLDET_OK;
    };
    if (fused_s_has_stamps() && choice == 2) {
        // the fold kernel's stamped build (-DSYLDET_S_STAMPS): shader clocks its waves spend waiting, summed over all waves in
        // 16 words, and behind them one record of four words a wave slot of the grid (kernels_fused_s.hip writes them):
        //   [0] hardware id register | XCC id << 32 | wave << 40 | waves a workgroup << 44
        //   [1], [2] the 100 MHz clock at the wave's entry and after its last tile     [3] its tiles | workgroup << 32
        // (a wave without a segment leaves zeros).  SYLDET_FUSED_STAMPS_FILE=<path>: the records as text, one line a wave
        // (tools/wave_skew.py reads them).
        const int64_t segs = (E + d.s_seg_evals - 1) / d.s_seg_evals;
        const size_t n_rec = (size_t)(segs + 8) * (size_t)C;
        if (int st = launch(16 + 4 * n_rec, "fused_s_kernel")) return st;
        const double w = (double)host[4], tl = (double)host[3];
        std::fprintf(stderr, "[syldet stamps] fold kernel: %.0f waves, %.1f tiles each; per tile: %.0f clocks in all, %.0f waiting for the samples' DMA (%.1f %%), "
                             "%.0f waiting for the LDS reads of the samples (%.1f %%)\n",
                     w, tl / w, (double)host[0] / tl, (double)host[1] / tl, 100.0 * (double)host[1] / (double)host[0], (double)host[2] / tl,
                     100.0 * (double)host[2] / (double)host[0]);
        if (const char *path = std::getenv("SYLDET_FUSED_STAMPS_FILE")) {
            if (FILE *f = std::fopen(path, "w")) {
                std::fprintf(f, "# workgroup wave waves hw_id xcc_id begin_10ns end_10ns tiles\n");
                for (size_t r = 0; r < n_rec; r++) {
                    const unsigned long long *q = host.data() + 16 + 4 * r;
                    if ((q[3] & 0xffffffffull) == 0) continue;
                    std::fprintf(f, "%llu %llu %llu %llu %llu %llu %llu %llu\n", q[3] >> 32, (q[0] >> 40) & 15, (q[0] >> 44) & 15, q[0] & 0xffffffffull,
                                 (q[0] >> 32) & 15, q[1], q[2], q[3] & 0xffffffffull);
                }
                std::fclose(f);
            }
        }
        return SYLDET_OK;
    }
    const bool rk = fused_r_applicable(d) && fused_r_has_stamps() && !h->sw.fused_classic;   // which kernel the launcher picks
    const int64_t seg = rk ? d.r_seg_evals : d.seg_evals;
    const size_t n = (size_t)((E + seg - 1) / seg) * (size_t)C * 16;
    if (int st = launch(n, "fused_kernel")) return st;
    double sum[16] = {0};
    for (size_t i = 0; i < n; i++) sum[i % 16] += (double)host[i];
    double tot = 0;
    for (int i = 0; i < 6; i++) tot += sum[i];            // wave 0's phases add up to the pass; wave 7's are a second view
    const char *names[16] = {"DFT(p) || evaluate(p-1) || block max(p+1)", "barrier 1", "carry + mag + columns", "stage next pass + issue loads",
                                    "barrier 0", "-", "-", "-", "wave 7: DFT || evaluate || block max", "wave 7: barrier 1", "wave 7: carry + mag + columns",
                                    "wave 7: stage + issue loads", "wave 7: barrier 0", "-", "-", "-"};
    if (rk) {
        names[0] = "top of the pass (scale, first fragments)"; names[1] = "ticks 0-23 (stage || evaluate: MFMA phase)";
        names[2] = "ticks 24-47 (stage || evaluate: MFMA phase)"; names[3] = "ticks 48-71 (evaluate: vector phase, magnitudes)";
        names[4] = "ticks 72-95 (magnitudes, block max, strip)"; names[5] = "barrier";
        for (int i = 0; i < 6; i++) names[8 + i] = names[i];
        d.runs = d.r_runs;
    }
    std::fprintf(stderr, "[syldet stamps] runs=%d workgroups=%zu cycles/pass=%.0f\n", d.runs, n / 16, tot / ((double)(n / 16) * d.runs));
    for (int i = 0; i < 16; i++)
        if (sum[i] > 0 && i % 8 < 6) std::fprintf(stderr, "   %-32s %6.0f cycles/pass  %5.1f %%\n", names[i], sum[i] / ((double)(n / 16) * d.runs), 100.0 * sum[i] / tot);
    if (sum[7] > 0)       // (the register-resident-basis kernel's stamped build: whole segments in both clocks)
        std::fprintf(stderr, "   segment: %.0f shader clocks in %.2f us: %.3f GHz\n", sum[6] / (double)(n / 16), sum[7] / (double)(n / 16) * 0.01, sum[6] / (sum[7] * 10.0));
    return SYLDET_OK;
}

// Launches a batch by its route `r` (any family but kMixed) on rows that are already what the route reads.
// d_net_of: a multi-network handle's network of each of the C rows (null: the handle's own [C] table, rows = channels).
// d_row_of: a mixed bank's class launch, the bank row of each of the C channels (null: row c).
int run_route(syldet *h, const Route &r, Samples x, int64_t S, int64_t stride, int C, float *d_outputs, uint8_t *d_flags, hipStream_t stream,
              const int *d_net_of, const int *d_row_of)
{
    const int64_t J = r.J, E = r.E;
    if (E <= 0) return SYLDET_OK;
    const float *d_samples = (const float *)x.p;      // (x.s16 from here on: int16 rows, read by the fold kernel's s16 form alone)
    // the network stage's (and the exact recomputation's) view of the rows' networks and of the bank's rows
    NetDesc net = h->net;
    net.row_of = d_row_of;
    FusedMulti mn{h->fnets, nullptr, d_row_of};
    if (h->n_nets > 1) {
        net.net_of = mn.net_of = d_net_of ? d_net_of : (const int *)h->d_net_of.ptr;
    } else if (h->fnets) {
        mn.net_of = (const int *)h->d_net_of.ptr;     // (a mixed bank's one-network class on the fold kernel: all zeros)
    }
    const FusedMulti *mnp = h->fnets ? &mn : nullptr;
    if (r.family == Route::kFused) {
        FusedDesc d = r.d;
        if (h->sw.fused_stamps) return run_stamped(h, d, r.choice, d_samples, stride, C, S, J, E, d_outputs, d_flags, stream);
        // the precision guard's work list, and behind the fused kernel the exact recomputation of what it reports
        const int64_t segs = (E + d.r_seg_evals - 1) / d.r_seg_evals + (E + d.seg_evals - 1) / d.seg_evals +
                             (d.s_seg_evals > 0 ? (E + d.s_seg_evals - 1) / d.s_seg_evals : 0);
        if (int st = prepare_fix(h, C, E, segs, stream, d.fix)) return st;
        {
            // (the launcher picks the register-resident-basis kernel where it is instantiated: named for what runs)
            static const char *const names[3] = {"fused_kernel", "fused_r_kernel", "fused_s_kernel"};
            KernelTimer t(h, stream, names[r.choice]);
            SYLDET_HIP(launch_fused(d, d_samples, stride, C, S, J, E, d_outputs, d_flags, stream, mnp, x.s16));
            note_call(h, true);
        }
        FixDesc fd = h->fixd;
        fd.s16 = x.s16 ? 1 : 0;                      // (the exact recomputation reads the same rows)
        return timed_fixup(h, stream, d.fix, [&](const FixList &l) { return launch_fixup(fd, net, d_samples, stride, J, E, d_outputs, d_flags, nullptr, l, stream); });
    }
    // (+ 16 bytes: the matrix-core network stage reads a frame's last bins as a whole quad)
    if (int st = h->d_columns.reserve((size_t)C * (size_t)J * (size_t)h->geom.bins * sizeof(float) + 16)) return st;
    switch (r.family) {
    case Route::kWide: {
        if (!h->wide.front)
            if (int st = h->d_xn.reserve((size_t)C * (size_t)E * (size_t)kWideK * 2)) return st;
        if (int st = stft_on_stream(h, d_samples, stride, C, J, (float *)h->d_columns.ptr, stream)) return st;
        if (!h->wide.front) {
            KernelTimer t(h, stream, wide_prep_is_chain(h->net) ? "wide_prep_chain_kernel" : "wide_prep_kernel");
            SYLDET_HIP(launch_wide_prep(h->net, h->geom.bins, (const float *)h->d_columns.ptr, C, J, E, h->d_xn.ptr, stream));
        }
        KernelTimer t(h, stream, h->wide.m32 ? "wide_gemm32s_kernel" : (h->wide.shape16 ? "wide_gemm16_kernel" : "wide_gemm_kernel"));
        SYLDET_HIP(launch_wide_gemm(h->wide, h->d_xn.ptr, (const float *)h->d_columns.ptr, J, E, (int64_t)C * E, d_outputs, d_flags, stream));
        return SYLDET_OK;
    }
    case Route::kBdft: {
        KernelTimer t(h, stream, "bdft_net_kernel");
        SYLDET_HIP(launch_bdft_net(h->bdft.md, h->bdft.desc, d_samples, stride, C, S, J, E, d_outputs, d_flags, stream));
        return SYLDET_OK;
    }
    case Route::kFft1k: {
        KernelTimer t(h, stream, "fft1k_net_kernel");
        SYLDET_HIP(launch_fft1k_net(h->stft, h->mlpx.desc, d_samples, stride, C, J, E, d_outputs, d_flags, stream));
        return SYLDET_OK;
    }
    default: break;             // kColumns
    }
    if (int st = stft_on_stream(h, d_samples, stride, C, J, (float *)h->d_columns.ptr, stream, true, d_row_of)) return st;
    if (h->mlpx.ok && (uint64_t)E * 4u < 0xFFFFFFF0ull) {
        KernelTimer t(h, stream, "mlp_mfma_kernel");
        SYLDET_HIP(launch_mlpx(h->mlpx.desc, (const float *)h->d_columns.ptr, C, J, E, d_outputs, d_flags, stream));
        return SYLDET_OK;
    }
    {
        KernelTimer t(h, stream, "mlp_generic_kernel");
        SYLDET_HIP(launch_mlp_generic(net, h->geom.bins, (const float *)h->d_columns.ptr, C, J, E, d_outputs,
                                      d_flags, stream));
    }
    return SYLDET_OK;
}
}  // namespace

namespace sd {

void forget_call(const syldet *h)
{
    if (t_last_call.h == h) t_last_call = LastCall();     // (the next handle may get this address)
}

void apply_switches(const syldet::Switches &sw, FusedDesc &d)
{
    d.stamps = nullptr;                            // (run_stamped sets them)
    d.ko = sw.fused_ko;                            // diagnostic only: SYLDET_FUSED_KO=<mask> runs an instantiation with parts of the kernel knocked out
    d.force_classic = sw.fused_classic ? 1 : 0;
    d.no_fold = sw.fused_nofold ? 1 : 0;
    d.no_fold2 = sw.fused_nofold2 ? 1 : 0;
    if (sw.fused_nohopk) d.s_hopk_rc = 0;
    if (sw.fused_nopairstep) d.s_pairstep = 0;
    d.no_cs8 = sw.fused_pad128 ? 1 : 0;
}

// One batch on a stream: its route, 16-bit PCM rows widened unless the route reads them natively (through one copy: DESIGN §4.11),
// the launch.  d_net_of, d_row_of: run_route's.
int run_on_stream(syldet *h, Samples x, int64_t S, int64_t stride, int C, float *d_outputs, uint8_t *d_flags, hipStream_t stream,
                  const int *d_net_of, const int *d_row_of)
{
    const uintptr_t base = reinterpret_cast<uintptr_t>(x.p);
    const Route r = route_for(h, S, stride, C, x.s16, base);
    if (r.family == Route::kNone) return SYLDET_OK;
    SYLDET_HIP(hipSetDevice(h->device));
    if (!h->root) h->prof_begin();                   // (a class handle's launches belong to its bank's call)
    if (!h->root) note_call(h, false);
    if (r.family != Route::kMixed) {
        if (x.s16 && !r.native_s16)
            if (int st = widen_s16(h, x, S, stride, C, stream)) return st;
        return run_route(h, r, x, S, stride, C, d_outputs, d_flags, stream, d_net_of, d_row_of);
    }
    // a mixed bank over all its channels: each class in turn, in place through its row table.  16-bit PCM: a class on the
    // fold kernel's s16 form reads the int16 rows in place; the others share one widened copy, made at most once a call.
    if (C != h->channels) return fail(SYLDET_ERR_INVALID_ARGUMENT, "a mixed bank's batch covers all its channels");
    Samples wide = x;
    int64_t wstride = stride;
    for (auto &k : h->classes) {
        const Route rk = route_for(k.get(), S, stride, k->channels, x.s16, base);
        const bool widen = x.s16 && !rk.native_s16;
        if (widen && wide.s16)
            if (int st = widen_s16(h, wide, S, wstride, C, stream)) return st;
        if (int st = run_route(k.get(), rk, widen ? wide : x, S, widen ? wstride : stride, k->channels, d_outputs, d_flags, stream, nullptr,
                               (const int *)k->d_row_of.ptr))
            return st;
    }
    return SYLDET_OK;
}

int interleaved_args(const syldet *h, int64_t n_frames, int32_t total_channels)
{
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (total_channels != h->channels) return fail(SYLDET_ERR_INVALID_ARGUMENT, "total_channels must equal the bank's channel count");
    if (n_frames < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_frames must be >= 0");
    return SYLDET_OK;
}

}  // namespace sd

extern "C" {

int64_t syldet_segment_evals(const syldet_t *h, int64_t n_samples)
{
    if (!h || h->engine != SYLDET_ENGINE_FUSED) return 0;
    const int64_t E = count_evals(h, n_samples);
    if (E <= 0) return 0;
    FusedDesc d = h->fused.desc;
    fused_segmentation(d, E, h->channels);
    apply_switches(h->sw, d);
    const int choice = fused_choice(d, count_frames(h, n_samples));
    return choice == 2 ? d.s_seg_evals : (choice == 1 ? d.r_seg_evals : d.seg_evals);
}

int syldet_last_fused_form(const syldet_t *h, int32_t *kernel, int32_t params[10])
{
    if (!h || !kernel || !params) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (t_last_call.h != h || !t_last_call.fused) return fail(SYLDET_ERR_UNSUPPORTED, "this thread's last call through the handle ran no fused kernel");
    *kernel = t_last_call.form.kernel;
    for (int i = 0; i < 10; i++) params[i] = t_last_call.form.p[i];
    return SYLDET_OK;
}

int32_t syldet_fused_dry_run_active(void) { return fused_seam().dry ? 1 : 0; }

int syldet_fused_form_of_config(const syldet_config_t *const *cfgs, int32_t n_nets, const int32_t *channel_net, int32_t n_channels,
                                int64_t n_samples, int32_t s16, int32_t spectrogram, int32_t engine, int32_t *kernel, int32_t params[10])
{
    if (!cfgs || !kernel || !params) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_nets < 1 || (n_nets > 1 && !channel_net)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_nets must be >= 1, with a channel_net for more than one");
    if (n_channels <= 0 || n_channels > 65535) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_channels must be in [1, 65535]");
    if (n_samples < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_samples must be >= 0");
    if (!engine_known(engine)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "unknown engine");
    for (int32_t i = 0; i < n_nets; i++)
        if (!cfgs[i]) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL configuration " + std::to_string(i));
    const bool multi = channel_net != nullptr && n_nets > 1;
    for (int32_t c = 0; multi && c < n_channels; c++)
        if (channel_net[c] < 0 || channel_net[c] >= n_nets) return fail(SYLDET_ERR_INVALID_ARGUMENT, "channel_net entry outside [0, n_nets)");
    // the launchers run dry from here to the end of the call, whichever way it ends
    struct Dry {
        Dry() { fused_seam().dry = true; fused_seam().last.kernel = -1; }
        ~Dry() { fused_seam().dry = false; }
    } dry;
    // a handle as the create calls make it, as far as the host goes: configuration, geometry, switches, engine, plans
    int asked = engine;
    bool on_fold = false;
    if (multi) {
        if (engine == SYLDET_ENGINE_WIDE_BF16) return fail(SYLDET_ERR_UNSUPPORTED, "the wide-network engine has no multi-network form");
        std::vector<std::unique_ptr<OwnedConfig>> own;
        bool fold = true, fused_ok = true;
        if (int st = survey_nets(cfgs, n_nets, own, fold, fused_ok)) return st;
        if (engine == SYLDET_ENGINE_FUSED && !fused_ok)
            return fail(SYLDET_ERR_UNSUPPORTED, "fused engine on a multi-network handle: only the fold kernel has that form, and it does not take this shape");
        on_fold = engine == SYLDET_ENGINE_FUSED || (engine == SYLDET_ENGINE_AUTO && fold);
        if (!on_fold) asked = SYLDET_ENGINE_GENERIC;
    }
    std::unique_ptr<syldet> h(new (std::nothrow) syldet());
    if (!h) return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    if (int st = h->cfg.assign(*cfgs[0])) return st;
    if (int st = compute_geometry(h->cfg.view, &h->geom)) return st;
    h->sw.read();
    h->channels = n_channels;
    if (int st = choose_engine(h.get(), asked)) return st;
    static const FusedNet no_tables{};                     // (never read: a multi-network handle's tables are on the device)
    if (multi) {
        h->n_nets = n_nets;
        if (on_fold) {
            if (h->engine != SYLDET_ENGINE_FUSED) return fail(SYLDET_ERR_UNSUPPORTED, "the fold kernel did not take network 0");
            h->fnets = &no_tables;
        }
    }
    const int C = n_channels;
    const int64_t S = n_samples, J = count_frames(h.get(), S), E = count_evals(h.get(), S);
    FusedDesc d{};
    hipError_t e = hipSuccess;
    if (spectrogram) {
        if (multi) return fail(SYLDET_ERR_UNSUPPORTED, "the transform's form is asked of one configuration");
        if (J <= 0) return fail(SYLDET_ERR_UNSUPPORTED, "not on the fused engine: no frame in n_samples");
        if (asked != SYLDET_ENGINE_GENERIC && plan_dft(h.get())) {
            h->dft.desc.spect_power = h->cfg.view.spectrum == SYLDET_SPECTRUM_MAGNITUDE ? 1 : 0;
            h->has_dft = true;
        }
        bool fold = false;
        static float no_columns;                           // (never written: the launcher wants a destination)
        if (!dft_route_for(h.get(), J, C, false, nullptr, &no_columns, d, fold))
            return fail(SYLDET_ERR_UNSUPPORTED, "not on the fused engine: the transform keeps the generic FFT");
        e = fold ? launch_fused_s_spectrogram(d, nullptr, S, C, J, nullptr) : launch_fused_spectrogram(d, nullptr, S, C, J, nullptr);
    } else {
        if (E <= 0) return fail(SYLDET_ERR_UNSUPPORTED, "not on the fused engine: no evaluation in n_samples");
        if (h->sw.fused_stamps) return fail(SYLDET_ERR_UNSUPPORTED, "SYLDET_FUSED_STAMPS: the diagnostic instantiations are not reported");
        // (rows at an aligned address, an even stride apart: run_on_stream's own route, then its launcher, dry)
        const int64_t stride = (S + 1) & ~(int64_t)1;
        const Route r = route_for(h.get(), S, stride, C, s16 != 0, 0);
        if (r.family != Route::kFused)
            return fail(SYLDET_ERR_UNSUPPORTED, "not on the fused engine" + (h->fused.reason.empty() ? std::string() : ": " + h->fused.reason));
        FusedMulti mn{h->fnets, nullptr, nullptr};
        e = launch_fused(r.d, nullptr, stride, C, S, J, E, nullptr, nullptr, nullptr, h->fnets ? &mn : nullptr, r.native_s16);
    }
    if (e != hipSuccess) return fail(SYLDET_ERR_UNSUPPORTED, "not on the fused engine: no instantiation takes the plan");
    const FusedForm &f = fused_seam().last;
    if (f.kernel < 0) return fail(SYLDET_ERR_UNSUPPORTED, "not on the fused engine: the launcher ran nothing");
    *kernel = f.kernel;
    for (int i = 0; i < 10; i++) params[i] = f.p[i];
    return SYLDET_OK;
}

int syldet_run_device(syldet_t *h, const float *d_samples, int64_t n_samples, int64_t channel_stride, float *d_outputs,
                      uint8_t *d_flags, void *hip_stream)
{
    if (int st = check_batch_args(h, d_samples, n_samples, channel_stride)) return st;
    return run_on_stream(h, d_samples, n_samples, channel_stride, h->channels, d_outputs, d_flags, (hipStream_t)hip_stream);
}

int syldet_run_device_s16(syldet_t *h, const int16_t *d_samples, int64_t n_samples, int64_t channel_stride, float *d_outputs,
                          uint8_t *d_flags, void *hip_stream)
{
    if (int st = check_batch_args(h, d_samples, n_samples, channel_stride)) return st;
    return run_on_stream(h, Samples(d_samples, true), n_samples, channel_stride, h->channels, d_outputs, d_flags, (hipStream_t)hip_stream);
}

int syldet_spectrogram_device(syldet_t *h, const float *d_samples, int64_t n_samples, int64_t channel_stride,
                              float *d_columns, void *hip_stream)
{
    if (int st = check_batch_args(h, d_samples, n_samples, channel_stride)) return st;
    if (h->classes.size() > 1) return fail(SYLDET_ERR_UNSUPPORTED, "spectrogram of a mixed bank: its classes' columns are ragged");
    if (!d_columns) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    SYLDET_HIP(hipSetDevice(h->device));
    const int64_t J = count_frames(h, n_samples);
    h->prof_begin();
    note_call(h, false);
    return stft_on_stream(h->classes.empty() ? h : h->classes[0].get(), d_samples, channel_stride, h->channels, J, d_columns, (hipStream_t)hip_stream, false);
}

int syldet_detections_device(syldet_t *h, const uint8_t *d_flags, int64_t n_evals, double debounce_seconds,
                             int64_t *d_indices, int64_t capacity, int64_t *d_counts, void *hip_stream)
{
    if (!h || !d_flags || n_evals < 0 || capacity < 0 || (capacity > 0 && !d_indices))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    SYLDET_HIP(hipSetDevice(h->device));
    const int64_t debounce_frames = (int64_t)(debounce_seconds * h->cfg.view.sampling_rate);   // TrackDetector.swift:19-26
    SYLDET_HIP(launch_detections(d_flags, h->channels, n_evals, h->geom.first_index, h->geom.hop, debounce_frames,
                                 d_indices, capacity, d_counts, (hipStream_t)hip_stream));
    return SYLDET_OK;
}

// ---- host-pointer conveniences: stage, run, copy back, block ----

static int pipe_bring_up(syldet *h)
{
    syldet::Pipe &p = h->pipe;
    if (p.up) return SYLDET_OK;
    if (!p.s_in) SYLDET_HIP(hipStreamCreateWithFlags(&p.s_in, hipStreamNonBlocking));
    if (!p.s_out) SYLDET_HIP(hipStreamCreateWithFlags(&p.s_out, hipStreamNonBlocking));
    for (int b = 0; b < 2; b++)
        for (hipEvent_t *e : {&p.ev_h2d[b], &p.ev_k[b], &p.ev_d2h[b]})
            if (!*e) SYLDET_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    p.up = true;
    return SYLDET_OK;
}

// The batch call on host buffers: TrackDetector's loop reads a recording buffer by buffer and runs the detector on each
// (TrackDetector.swift:45-105); here the recording is cut along time into stages of about host_chunk_bytes of input, each
// stage the evaluations [e0, e0 + n) of every channel with the samples they reach ((n + T - 2) hop + gap + W: the halo of
// (T - 1) hop + W - hop samples is read by both neighbours), and the stages flow through two sets of device buffers: the H2D
// copy of stage k + 1 (copy-in stream) runs under the kernel of stage k (the handle's stream) and the D2H copy of stage k - 1
// (copy-out stream).  Device staging is bounded by two stages, whatever the recording's length.  Kernels whose scales
// are per frame or per hop-aligned block (the fold kernel, the FFT and block-transform engines) give a stage's evaluations
// the bits the one-shot call gives them; the pass-scaled kernels agree to a few 1e-7, as between any two tilings (syldet.h,
// syldet_fixup_stats).  The copies read and write the caller's rows in place: page-locked memory (syldet_host_alloc) is
// truly asynchronous; for ordinary memory the runtime pins the pages of each copy on the fly and the copy call returns when
// its bytes have moved -- the kernel of the stage before runs meanwhile all the same (measured: within a few per cent of
// the PCIe rate either way, and a staging copy through a pinned buffer of our own was half as fast).
// 16-bit PCM (syldet_run_s16) takes the same stages -- n_c from the fp32 byte count, so that the pass-scaled kernels see the
// tiling of syldet_run and give its bits -- with int16 staging: the copies in move half the bytes.
static int run_host(syldet *h, Samples x, int64_t n_samples, int64_t channel_stride, float *outputs, uint8_t *flags)
{
    const size_t es = x.s16 ? sizeof(int16_t) : sizeof(float);    // bytes a sample in the caller's rows and the device stages
    const char *samples = (const char *)x.p;
    std::lock_guard<std::mutex> staging(h->pump_mu);   // the staging buffers and h->stream: one user at a time
    SYLDET_HIP(hipSetDevice(h->device));
    const int C = h->channels, n_out = h->geom.outputs, T = h->cfg.view.time_range;
    const int64_t E = count_evals(h, n_samples), hop = h->geom.hop, frame = (int64_t)h->geom.gap + h->cfg.view.window_length;
    if (E <= 0) return SYLDET_OK;
    if (int st = pipe_bring_up(h)) return st;
    syldet::Pipe &p = h->pipe;

    // evaluations per stage: about host_chunk_bytes of input, the stages of equal size
    const int64_t fixed = (int64_t)C * ((T - 2) * hop + frame) * 4, per_eval = (int64_t)C * hop * 4;
    int64_t n_c = ((int64_t)h->host_chunk_bytes - fixed) / per_eval;
    if (n_c < 1) n_c = 1;
    const int64_t n_stages = (E + n_c - 1) / n_c;
    n_c = (E + n_stages - 1) / n_stages;
    const int64_t S_max = (n_c + T - 2) * hop + frame;
    for (int b = 0; b < (n_stages > 1 ? 2 : 1); b++) {
        if (int st = p.d_in[b].reserve((size_t)C * (size_t)S_max * es)) return st;
        if (int st = p.d_out[b].reserve((size_t)C * (size_t)n_c * (size_t)n_out * 4)) return st;
        if (int st = p.d_fl[b].reserve((size_t)C * (size_t)n_c)) return st;
    }
    // whatever happens, nothing of this call is in flight when it returns
    struct Drain {
        syldet *h;
        ~Drain()
        {
            (void)hipStreamSynchronize(h->pipe.s_in);
            (void)hipStreamSynchronize(h->stream);
            (void)hipStreamSynchronize(h->pipe.s_out);
        }
    } drain{h};

    for (int64_t k = 0; k < n_stages; k++) {
        const int b = (int)(k & 1);
        const int64_t e0 = k * n_c, n = std::min(n_c, E - e0), s0 = e0 * hop, Sc = (n + T - 2) * hop + frame;
        if (k >= 2) SYLDET_HIP(hipStreamWaitEvent(p.s_in, p.ev_k[b], 0));      // the kernel of stage k - 2 has read this device buffer
        SYLDET_HIP(hipMemcpy2DAsync(p.d_in[b].ptr, (size_t)Sc * es, samples + (size_t)s0 * es, (size_t)channel_stride * es, (size_t)Sc * es,
                                    (size_t)C, hipMemcpyHostToDevice, p.s_in));
        SYLDET_HIP(hipEventRecord(p.ev_h2d[b], p.s_in));
        SYLDET_HIP(hipStreamWaitEvent(h->stream, p.ev_h2d[b], 0));
        if (k >= 2) SYLDET_HIP(hipStreamWaitEvent(h->stream, p.ev_d2h[b], 0)); // stage k - 2's results have left the device buffers
        if (int st = run_on_stream(h, Samples(p.d_in[b].ptr, x.s16), Sc, Sc, C, (float *)p.d_out[b].ptr, (uint8_t *)p.d_fl[b].ptr, h->stream)) return st;
        SYLDET_HIP(hipEventRecord(p.ev_k[b], h->stream));
        SYLDET_HIP(hipStreamWaitEvent(p.s_out, p.ev_k[b], 0));
        if (outputs)
            SYLDET_HIP(hipMemcpy2DAsync(outputs + (size_t)e0 * n_out, (size_t)E * n_out * 4, p.d_out[b].ptr, (size_t)n * n_out * 4,
                                        (size_t)n * n_out * 4, (size_t)C, hipMemcpyDeviceToHost, p.s_out));
        if (flags)
            SYLDET_HIP(hipMemcpy2DAsync(flags + e0, (size_t)E, p.d_fl[b].ptr, (size_t)n, (size_t)n, (size_t)C, hipMemcpyDeviceToHost, p.s_out));
        SYLDET_HIP(hipEventRecord(p.ev_d2h[b], p.s_out));
    }
    SYLDET_HIP(hipStreamSynchronize(p.s_out));
    return SYLDET_OK;
}

int syldet_run(syldet_t *h, const float *samples, int64_t n_samples, int64_t channel_stride, float *outputs, uint8_t *flags)
{
    if (int st = check_batch_args(h, samples, n_samples, channel_stride)) return st;
    return run_host(h, samples, n_samples, channel_stride, outputs, flags);
}

int syldet_run_s16(syldet_t *h, const int16_t *samples, int64_t n_samples, int64_t channel_stride, float *outputs, uint8_t *flags)
{
    if (int st = check_batch_args(h, samples, n_samples, channel_stride)) return st;
    return run_host(h, Samples(samples, true), n_samples, channel_stride, outputs, flags);
}

// ---- interleaved (frame-major) audio: de-interleave on the device, then the batch path ----

// fp32 or (s16) int16 frames: the planar copy keeps the caller's sample width, then the batch path on it
static int run_interleaved_device(syldet *h, Samples x, int64_t n_frames, float *d_outputs, uint8_t *d_flags, hipStream_t stream)
{
    if (count_evals(h, n_frames) <= 0) return SYLDET_OK;
    if (!x.p) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL buffer");
    SYLDET_HIP(hipSetDevice(h->device));
    const int C = h->channels;
    if (int st = h->d_planar.reserve((size_t)C * (size_t)n_frames * (x.s16 ? sizeof(int16_t) : sizeof(float)))) return st;
    if (x.s16)
        SYLDET_HIP(launch_deinterleave_s16((const int16_t *)x.p, n_frames, C, C, (int16_t *)h->d_planar.ptr, n_frames, stream));
    else
        SYLDET_HIP(launch_deinterleave((const float *)x.p, n_frames, C, 0, C, (float *)h->d_planar.ptr, n_frames, stream));
    return run_on_stream(h, Samples(h->d_planar.ptr, x.s16), n_frames, n_frames, C, d_outputs, d_flags, stream);
}

int syldet_run_interleaved_device(syldet_t *h, const float *d_interleaved, int64_t n_frames, int32_t total_channels,
                                  float *d_outputs, uint8_t *d_flags, void *hip_stream)
{
    if (int st = interleaved_args(h, n_frames, total_channels)) return st;
    return run_interleaved_device(h, d_interleaved, n_frames, d_outputs, d_flags, (hipStream_t)hip_stream);
}

int syldet_run_interleaved_device_s16(syldet_t *h, const int16_t *d_interleaved, int64_t n_frames, int32_t total_channels,
                                      float *d_outputs, uint8_t *d_flags, void *hip_stream)
{
    if (int st = interleaved_args(h, n_frames, total_channels)) return st;
    return run_interleaved_device(h, Samples(d_interleaved, true), n_frames, d_outputs, d_flags, (hipStream_t)hip_stream);
}

static int run_interleaved_host(syldet *h, Samples x, int64_t n_frames, float *outputs, uint8_t *flags)
{
    const int C = h->channels;
    const int64_t E = count_evals(h, n_frames);
    if (E <= 0) return SYLDET_OK;
    if (!x.p) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL buffer");
    std::lock_guard<std::mutex> staging(h->pump_mu);   // the staging buffers and h->stream: one user at a time
    SYLDET_HIP(hipSetDevice(h->device));
    const size_t in_bytes = (size_t)C * (size_t)n_frames * (x.s16 ? sizeof(int16_t) : sizeof(float));
    const size_t out_bytes = (size_t)C * (size_t)E * (size_t)h->geom.outputs * sizeof(float);
    const size_t fl_bytes = (size_t)C * (size_t)E;
    if (int st = h->d_stage_in.reserve(in_bytes)) return st;
    if (int st = h->d_stage_out.reserve(out_bytes)) return st;
    if (int st = h->d_stage_flags.reserve(fl_bytes)) return st;
    SYLDET_HIP(hipMemcpyAsync(h->d_stage_in.ptr, x.p, in_bytes, hipMemcpyHostToDevice, h->stream));
    if (int st = run_interleaved_device(h, Samples(h->d_stage_in.ptr, x.s16), n_frames, (float *)h->d_stage_out.ptr,
                                        (uint8_t *)h->d_stage_flags.ptr, h->stream))
        return st;
    if (outputs) SYLDET_HIP(hipMemcpyAsync(outputs, h->d_stage_out.ptr, out_bytes, hipMemcpyDeviceToHost, h->stream));
    if (flags) SYLDET_HIP(hipMemcpyAsync(flags, h->d_stage_flags.ptr, fl_bytes, hipMemcpyDeviceToHost, h->stream));
    SYLDET_HIP(hipStreamSynchronize(h->stream));
    return SYLDET_OK;
}

int syldet_run_interleaved(syldet_t *h, const float *interleaved, int64_t n_frames, int32_t total_channels, float *outputs,
                           uint8_t *flags)
{
    if (int st = interleaved_args(h, n_frames, total_channels)) return st;
    return run_interleaved_host(h, interleaved, n_frames, outputs, flags);
}

int syldet_run_interleaved_s16(syldet_t *h, const int16_t *interleaved, int64_t n_frames, int32_t total_channels, float *outputs,
                               uint8_t *flags)
{
    if (int st = interleaved_args(h, n_frames, total_channels)) return st;
    return run_interleaved_host(h, Samples(interleaved, true), n_frames, outputs, flags);
}

int syldet_spectrogram(syldet_t *h, const float *samples, int64_t n_samples, int64_t channel_stride, float *columns)
{
    if (int st = check_batch_args(h, samples, n_samples, channel_stride)) return st;
    if (h->classes.size() > 1) return fail(SYLDET_ERR_UNSUPPORTED, "spectrogram of a mixed bank: its classes' columns are ragged");
    if (!columns) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> staging(h->pump_mu);   // the staging buffers and h->stream: one user at a time
    SYLDET_HIP(hipSetDevice(h->device));
    const int C = h->channels;
    const int64_t J = count_frames(h, n_samples);
    if (J <= 0) return SYLDET_OK;
    syldet *sh = h->classes.empty() ? h : h->classes[0].get();    // (the one class of a mixed bank that has one)
    const size_t in_bytes = (size_t)C * (size_t)n_samples * sizeof(float);
    const size_t col_bytes = (size_t)C * (size_t)J * (size_t)sh->geom.bins * sizeof(float);
    if (int st = h->d_stage_in.reserve(in_bytes)) return st;
    if (int st = h->d_columns.reserve(col_bytes)) return st;
    SYLDET_HIP(hipMemcpy2DAsync(h->d_stage_in.ptr, (size_t)n_samples * sizeof(float), samples,
                                (size_t)channel_stride * sizeof(float), (size_t)n_samples * sizeof(float), (size_t)C,
                                hipMemcpyHostToDevice, h->stream));
    h->prof_begin();
    if (int st = stft_on_stream(sh, (const float *)h->d_stage_in.ptr, n_samples, C, J, (float *)h->d_columns.ptr, h->stream, false)) return st;
    SYLDET_HIP(hipMemcpyAsync(columns, h->d_columns.ptr, col_bytes, hipMemcpyDeviceToHost, h->stream));
    SYLDET_HIP(hipStreamSynchronize(h->stream));
    return SYLDET_OK;
}

int syldet_detections(syldet_t *h, const uint8_t *flags, int64_t n_evals, double debounce_seconds, int64_t *indices,
                      int64_t capacity, int64_t *counts)
{
    if (!h || !flags || !counts || n_evals < 0 || capacity < 0 || (capacity > 0 && !indices))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    std::lock_guard<std::mutex> staging(h->pump_mu);   // the staging buffers and h->stream: one user at a time
    SYLDET_HIP(hipSetDevice(h->device));
    const int C = h->channels;
    const size_t fl_bytes = std::max<size_t>((size_t)C * (size_t)n_evals, 1);
    const size_t idx_bytes = std::max<size_t>((size_t)C * (size_t)capacity * sizeof(int64_t), 8);
    if (int st = h->d_stage_flags.reserve(fl_bytes)) return st;
    if (int st = h->d_stage_idx.reserve(idx_bytes)) return st;
    if (int st = h->d_stage_cnt.reserve((size_t)C * sizeof(int64_t))) return st;
    if (n_evals > 0)
        SYLDET_HIP(hipMemcpyAsync(h->d_stage_flags.ptr, flags, (size_t)C * (size_t)n_evals, hipMemcpyHostToDevice, h->stream));
    if (int st = syldet_detections_device(h, (const uint8_t *)h->d_stage_flags.ptr, n_evals, debounce_seconds,
                                          capacity > 0 ? (int64_t *)h->d_stage_idx.ptr : nullptr, capacity,
                                          (int64_t *)h->d_stage_cnt.ptr, h->stream))
        return st;
    if (capacity > 0)
        SYLDET_HIP(hipMemcpyAsync(indices, h->d_stage_idx.ptr, (size_t)C * (size_t)capacity * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    SYLDET_HIP(hipMemcpyAsync(counts, h->d_stage_cnt.ptr, (size_t)C * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    SYLDET_HIP(hipStreamSynchronize(h->stream));
    return SYLDET_OK;
}

}  // extern "C"
