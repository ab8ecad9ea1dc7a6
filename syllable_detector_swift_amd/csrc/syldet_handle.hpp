// syldet_handle.hpp -- the handle (struct syldet) and what the host files that touch one share (not installed; no kernel
// file includes it: kernels.hpp stays the kernels' header).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "carve.hpp"
#include "fused_plan.hpp"
#include "kernels.hpp"
#include "sample_ring.hpp"
#include "syldet_internal.hpp"

using namespace sd;   // (a private header: every file that includes it is libsyldet's host side)

namespace sd {

struct DeviceBuffer {
    void *ptr = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return SYLDET_OK;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&ptr, bytes);
        if (e != hipSuccess) {
            ptr = nullptr;
            return fail(e == hipErrorOutOfMemory ? SYLDET_ERR_OUT_OF_MEMORY : SYLDET_ERR_DEVICE,
                        std::string("hipMalloc: ") + hipGetErrorString(e));
        }
        cap = bytes;
        return SYLDET_OK;
    }
    void release()
    {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

struct PinnedBuffer {
    void *ptr = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return SYLDET_OK;
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr;
        cap = 0;
        hipError_t e = hipHostMalloc(&ptr, bytes, hipHostMallocDefault);
        if (e != hipSuccess) {
            ptr = nullptr;
            return fail(SYLDET_ERR_OUT_OF_MEMORY, std::string("hipHostMalloc: ") + hipGetErrorString(e));
        }
        cap = bytes;
        return SYLDET_OK;
    }
    void release()
    {
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

}  // namespace sd

struct syldet {
    OwnedConfig cfg;
    syldet_geometry_t geom{};
    int channels = 0;
    int device = 0;
    int engine = SYLDET_ENGINE_GENERIC;
    int engine_asked = SYLDET_ENGINE_AUTO;      // what syldet_create was asked for (AUTO commits to the fused engine only for what it can hold to 1e-5)

    // Diagnostic switches (A/B runs, and the tests that hold two forms of a kernel against each other): read from the
    // environment ONCE, when the handle is created -- never on the launch path, and a handle keeps the form it was created for.
    struct Switches {
        bool fused_classic = false;   // SYLDET_FUSED_CLASSIC: the 8-wave fused kernel where both fused kernels take the shape
        bool no_fft1k = false;        // SYLDET_NO_FFT1K: 1024-point frames as two launches
        bool wide_no_front = false;   // SYLDET_WIDE_NO_FRONT: the wide engine's inputs through the preparation kernel and the bf16 image in HBM (rounds 1-2)
        bool wide_wg16 = false;       // SYLDET_WIDE_WG16: the wide engine's GEMM as one workgroup of 16 waves a CU (rounds 1-3), not two of 8
        bool wide_stagger = true;     // SYLDET_WIDE_NOSTAGGER: the two-workgroup GEMM WITHOUT waves 4-7 running one epilogue behind waves 0-3 (round 4's order)
        bool wide_dma_builtin = false;   // SYLDET_WIDE_DMA_BUILTIN: (unstaggered) the weight DMA through the compiler's builtin, not the assembly statement
        bool wide_tiles4 = false;     // SYLDET_WIDE_T4: the staggered GEMM as one workgroup a CU with four evaluation tiles a wave
        bool wide_m32 = false;        // SYLDET_WIDE_M32: the staggered wide GEMM on the 32x32x16 MFMA shape (round 6, an A/B form)
        bool wide_tanh_poly = false;  // SYLDET_WIDE_TANH_POLY: the wide GEMM's hidden TanSig / LogSig layer through a clamped odd polynomial (seven terms, packed fp32), no transcendentals
        bool wide_shape32 = false;    // SYLDET_WIDE_SHAPE32: the wide engine's GEMM on the 32x32x16 MFMA shape (rounds 1-2), not 16x16x32
        bool no_bdft = false;         // SYLDET_NO_BDFT: frames of four hops on the FFT kernels, not the block-transform kernel
        bool no_stft_lanes = false;   // SYLDET_NO_STFT_LANES: the LDS Stockham FFT instead of the lane-butterfly one
        bool no_guard = false;        // SYLDET_NO_GUARD: the precision guard off
        bool no_mlpx = false;         // SYLDET_NO_MLPX: the interpretive network kernels under AUTO
        bool fused_nofold = false;    // SYLDET_FUSED_NOFOLD: not the symmetric-fold kernel (the register-resident-basis / 8-wave kernels)
        bool fused_pad128 = false;    // SYLDET_FUSED_PAD128: hop 128 on the fold kernel's padded pieces, not the staggered chunks (round 6)
        bool fused_nofold2 = false;   // SYLDET_FUSED_NOFOLD2: the fold kernel's once-folded form where the twice-folded one takes the shape
        bool fused_nohopk = false;    // SYLDET_FUSED_HOPK=0: the fold kernel's run-time hop where the compile-time schedule (hop 132) takes the shape
        bool fused_nopairstep = false;   // SYLDET_FUSED_PAIRSTEP=0: the compile-time-hop form without the progress words that keep a SIMD's two waves in step
        bool fused_stamps = false;    // SYLDET_FUSED_STAMPS: the stamped diagnostic instantiation
        int fused_ko = 0;             // SYLDET_FUSED_KO=<mask>: knock-out instantiation
        long long host_chunk = 0;     // SYLDET_HOST_CHUNK_BYTES=<n>: bytes of input per stage of the host-pointer pipeline (tests force seams with it)
        void read()
        {
            host_chunk = std::getenv("SYLDET_HOST_CHUNK_BYTES") ? std::atoll(std::getenv("SYLDET_HOST_CHUNK_BYTES")) : 0;
            fused_classic = std::getenv("SYLDET_FUSED_CLASSIC") != nullptr;
            no_fft1k = std::getenv("SYLDET_NO_FFT1K") != nullptr;
            no_bdft = std::getenv("SYLDET_NO_BDFT") != nullptr;
            wide_shape32 = std::getenv("SYLDET_WIDE_SHAPE32") != nullptr;
            wide_wg16 = std::getenv("SYLDET_WIDE_WG16") != nullptr;
            wide_stagger = std::getenv("SYLDET_WIDE_NOSTAGGER") == nullptr;
            wide_dma_builtin = std::getenv("SYLDET_WIDE_DMA_BUILTIN") != nullptr;
            wide_tiles4 = std::getenv("SYLDET_WIDE_T4") != nullptr;
            wide_tanh_poly = std::getenv("SYLDET_WIDE_TANH_POLY") != nullptr;
            wide_m32 = std::getenv("SYLDET_WIDE_M32") != nullptr;
            wide_no_front = std::getenv("SYLDET_WIDE_NO_FRONT") != nullptr;
            no_stft_lanes = std::getenv("SYLDET_NO_STFT_LANES") != nullptr;
            no_guard = std::getenv("SYLDET_NO_GUARD") != nullptr;
            no_mlpx = std::getenv("SYLDET_NO_MLPX") != nullptr;
            fused_nofold = std::getenv("SYLDET_FUSED_NOFOLD") != nullptr;
            fused_nofold2 = std::getenv("SYLDET_FUSED_NOFOLD2") != nullptr;
            fused_nohopk = std::getenv("SYLDET_FUSED_HOPK") != nullptr && std::atoi(std::getenv("SYLDET_FUSED_HOPK")) == 0;
            fused_nopairstep = std::getenv("SYLDET_FUSED_PAIRSTEP") != nullptr && std::atoi(std::getenv("SYLDET_FUSED_PAIRSTEP")) == 0;
            fused_pad128 = std::getenv("SYLDET_FUSED_PAD128") != nullptr;
            fused_stamps = std::getenv("SYLDET_FUSED_STAMPS") != nullptr;
            fused_ko = std::getenv("SYLDET_FUSED_KO") ? std::atoi(std::getenv("SYLDET_FUSED_KO")) : 0;
        }
    } sw;

    // device tables
    DeviceBuffer d_window, d_tw, d_sw, d_params, d_thr;
    StftDesc stft{};
    NetDesc net{};

    // scratch
    DeviceBuffer d_columns;           // generic engine: [C][J][F]

    // fused engine tables
    FusedPlan fused;
    DeviceBuffer d_stamps;            // diagnostic stamps (SYLDET_FUSED_STAMPS)
    // precision guard of the fused kernels (kernels.hpp, FixItem): work list + what the exact recomputation needs
    DeviceBuffer d_fix;               // 8 counters | items
    DeviceBuffer d_ctab;              // [N] (cos, sin)(2 pi m / N) fp64
    FixDesc fixd{};
    bool has_fix = false;
    DeviceBuffer d_fused;             // one blob: dfrag | wfrag | koff | bias0 | rvec | w1 | b1 | out_params
    DeviceBuffer d_stage_in, d_stage_out, d_stage_flags, d_stage_idx, d_stage_cnt;
    DeviceBuffer d_planar;            // channel-major copy of interleaved input (syldet_run_interleaved*: fp32 or int16)
    DeviceBuffer d_widen;             // 16-bit PCM batches: the packed fp32 copy x * 2^-15 the engines read (widen_s16_kernel)

    // the fused engine's DFT front half as the STFT of the other engines (W <= 256, F <= 32, hop % 4 == 0)
    FusedPlan dft;
    DeviceBuffer d_dft;
    bool has_dft = false;

    // the generic engine's network stage on the matrix cores, where the configuration is of its class (kernels_mlpx.hip)
    MlpxPlan mlpx;
    DeviceBuffer d_mlpx;              // afrag | bias0 | w1
    // ... with the block-transform front (kernels_bdft.hip) where frames are four hops long
    BdftPlan bdft;
    DeviceBuffer d_bdft;              // basis | cre | afrag

    // wide-network engine (SYLDET_ENGINE_WIDE_BF16)
    WideDesc wide{};
    DeviceBuffer d_wide;              // packed first-layer chunks | b1 | output maps
    DeviceBuffer d_xn;                // [C*E][kWideK] bf16 normalised inputs
    hipStream_t stream = nullptr;     // used by the host-pointer entry points

    // multi-network handles (syldet_create_multi): channel c runs network net_of[c] of n_nets compatible ones.  cfg is network
    // 0's (the shape every network shares); the per-network tables sit at a fixed stride: the generic engine's parameter blobs
    // and thresholds (net.params_stride / thr_stride), and the fold kernel's FusedNet tables (d_fnets, fnets).
    int n_nets = 1;
    std::vector<int> net_of;          // [C] (empty for one network)
    std::vector<std::unique_ptr<OwnedConfig>> net_cfgs;   // [n_nets] every network's configuration (what syldet_trainer_create_multi reads)
    std::vector<double> chan_thr0;    // [C] the first threshold of each channel's network (syldet_last_detected)
    DeviceBuffer d_net_of;            // [C] int
    // the Simulator's trace (syldet_trace*): channel c divides by Float(thresholds[k]) of its own network
    std::vector<double> chan_thr;     // [C][outputs] every threshold of each channel's network (multi-network and mixed banks; empty: cfg's for all)
    std::vector<DeviceBuffer> d_trace_thr;   // [outputs] the [C] fp32 table of output k, made on the first trace of that output
    DeviceBuffer d_trace;             // the host forms' trace rows on the device
    // the TTL trigger track (syldet_trigger*; kernels_trigger.hip)
    DeviceBuffer d_trigger_last;      // last_seen [C][B'] int32: the scan's table, grown to the longest recording seen
    DeviceBuffer d_trigger;           // the host forms' track rows on the device
    // the level meters (syldet_levels*, syldet_output_levels*; kernels_levels.hip)
    DeviceBuffer d_levels_part;       // the partials of readings that cross workgroups (two a workgroup)
    DeviceBuffer d_levels;            // the host forms' readings on the device
    // ... and their streaming form (Processor.swift:111-113, :138, :158-184): two StatMax statistics a channel, off until
    // syldet_meters_enable.  The lock is the channel's own and is held for a comparison: writers (the producer's append, the
    // consumer's processNewValue) and the reader (any thread) never lose a value to each other.
    struct Meter {
        std::mutex mu;
        bool in_has = false, out_has = false;
        double in_cur = 0.0, out_cur = 0.0;
        static void write(bool &has, double &cur, double v)   // StatMax.writeValue: the first as it is, a later one if greater
        {
            if (!has) { cur = v; has = true; }
            else if (v > cur) cur = v;
        }
    };
    std::vector<std::unique_ptr<Meter>> meters;   // [C], made by the first syldet_meters_enable
    std::atomic<bool> meters_on{false};
    DeviceBuffer d_fnets;             // per-network fold-kernel tables, then FusedNet[n_nets]
    DeviceBuffer d_stage_net;         // [C] int: net_of of the channels one streaming launch carries
    const FusedNet *fnets = nullptr;  // (in d_fnets) null unless the handle runs the fold kernel's multi-network form

    // mixed banks (syldet_create_mixed): networks that share the evaluation clock and may differ in anything else.  They fall
    // into classes of compatible networks (syldet_config_compatible); each class is a handle of its own, in `classes`, made as
    // syldet_create_multi would make one for that class's networks over its channels.  A batch call launches the classes one
    // after another on the caller's stream, each reading and writing the bank's rows in place through its row table.  This
    // handle keeps the clock (cfg and geom: the first class's network, the fields that differ between classes set to -1), the
    // channels' streaming state, the stream and the profile.
    std::vector<std::unique_ptr<syldet, int (*)(syldet_t *)>> classes;
    std::vector<int> class_of, local_of;   // [C] a channel's class, and its index among that class's channels
    std::vector<int> bank_net;             // [C] the caller's channel_net (what syldet_recordings_plan's eligibility reads: sd::bank_info)
    // ... and in a class handle: its channels' bank rows, ascending, and the bank it belongs to (what the timers record into)
    std::vector<int> rows;
    DeviceBuffer d_row_of;            // [channels] int: rows
    syldet *root = nullptr;

    std::vector<std::unique_ptr<ChannelStream>> streams;
    std::mutex pump_mu;               // the staging buffers and the stream below belong to one pump at a time
    PinnedBuffer p_stage_in, p_stage_out;

    // the host-pointer batch call as a pipeline along time (syldet_run): two sets of device buffers, a copy-in and a copy-out
    // stream beside the compute stream, one event of each kind per set
    struct Pipe {
        hipStream_t s_in = nullptr, s_out = nullptr;
        DeviceBuffer d_in[2], d_out[2], d_fl[2];
        hipEvent_t ev_h2d[2] = {nullptr, nullptr}, ev_k[2] = {nullptr, nullptr}, ev_d2h[2] = {nullptr, nullptr};
        bool up = false;
    } pipe;
    size_t host_chunk_bytes = (size_t)256 << 20;   // SYLDET_HOST_CHUNK_BYTES (read at create): device staging per set

    // optional per-kernel timing (syldet_profile)
    bool profiling = false;
    // a ring of the last prof_depth batch calls: kMaxTimed kernel slots each, two events a slot
    static constexpr int kMaxTimed = 8;
    struct ProfCall { int count = 0; const char *names[kMaxTimed] = {}; bool fix = false; hipStream_t fix_stream = nullptr; };   // fix: the exact path was launched behind the call's kernels (on fix_stream)
    unsigned *prof_items_dev = nullptr;      // ... as the device addresses it
    unsigned *prof_items = nullptr;          // [prof_items_n] page-locked: the exact path's work items of each profiled call (timed_fixup)
    int prof_items_n = 0;
    std::vector<hipEvent_t> events;          // [prof_depth][kMaxTimed][2], created on first use
    std::vector<ProfCall> prof_calls;        // [prof_depth]
    int prof_depth = 1;
    int64_t prof_seq = 0;                    // batch calls profiled so far
    int prof_cur() const { return (int)((prof_seq > 0 ? prof_seq - 1 : 0) % prof_depth); }
    void prof_begin()                        // a batch call starts
    {
        if (!profiling) return;
        if ((int)prof_calls.size() != prof_depth) prof_calls.assign((size_t)prof_depth, ProfCall());
        prof_seq++;
        prof_calls[(size_t)prof_cur()].count = 0;
        prof_calls[(size_t)prof_cur()].fix = false;
        if (prof_items && prof_cur() < prof_items_n) prof_items[2 * prof_cur()] = prof_items[2 * prof_cur() + 1] = 0u;
    }
};

namespace sd {

// Brackets one kernel launch with events on its own stream when profiling is on.
struct KernelTimer {
    syldet *h;
    hipStream_t stream;
    int slot = -1;
    KernelTimer(syldet *h_, hipStream_t s, const char *name) : h(h_->root ? h_->root : h_), stream(s)   // (a class handle: its bank's profile)
    {
        if (!h->profiling || h->prof_calls.empty()) return;
        syldet::ProfCall &pc = h->prof_calls[(size_t)h->prof_cur()];
        if (pc.count >= syldet::kMaxTimed) return;
        slot = pc.count++;
        pc.names[slot] = name;
        base = (size_t)(h->prof_cur() * syldet::kMaxTimed + slot) * 2;
        if (h->events.size() < (size_t)h->prof_depth * syldet::kMaxTimed * 2) h->events.resize((size_t)h->prof_depth * syldet::kMaxTimed * 2, nullptr);
        for (int k = 0; k < 2; k++)
            if (!h->events[base + (size_t)k]) (void)hipEventCreate(&h->events[base + (size_t)k]);
        (void)hipEventRecord(h->events[base], stream);
    }
    ~KernelTimer()
    {
        if (slot >= 0) (void)hipEventRecord(h->events[base + 1], stream);
    }
    size_t base = 0;
};

// A batch's device samples as the caller passed them: fp32, or 16-bit PCM whose sample x means x * 2^-15 (the *_s16 entry
// points).  One route decision serves both (run_on_stream).
struct Samples {
    const void *p = nullptr;
    bool s16 = false;
    Samples(const float *f) : p(f) {}
    Samples(const void *q, bool pcm16) : p(q), s16(pcm16) {}
};

// What the handles that sit on a bank and, optionally, on a packed-recordings plan share (the scorer, the aligner, the trainer,
// the matchers): the bank, and the plan's detectors as spans of the handle's unit (detector_spans.hpp).
struct DetectorTable {
    syldet *h = nullptr;                     // the bank (it outlives the handle): its profile
    BankInfo bank{};
    bool packed = false;
    int D = 0;                               // detectors: the bank's channels, or (packed) the plan's recordings
    int64_t row_samples = 0, row_evals = 0;  // (packed) syldet_recordings_shape's
    int64_t row_units = 0;                   // (packed) a row's length in the spans' unit: what a call's row length must be
    std::vector<DetSpan> spans;              // (packed) [D] in the caller's order

    // the bank's clock and, of a plan (r may be NULL), its slots in `unit`, held once more to the plan's guarantee that no
    // recording reaches beyond its row
    int read(const syldet_t *bank_handle, const syldet_recordings_t *r, SpanUnit unit)
    {
        h = const_cast<syldet *>(bank_handle);
        bank_info(bank_handle, &bank);
        packed = r != nullptr;
        D = bank.channels;
        if (!r) return SYLDET_OK;
        int32_t K = 0;
        if (int st = syldet_recordings_shape(r, &K, &row_samples, &row_evals, nullptr)) return st;
        D = K;
        row_units = span_row_units(bank, unit, row_samples, row_evals);
        std::vector<syldet_slot_t> plan((size_t)D);
        if (D > 0)
            if (int st = syldet_recordings_slots(r, plan.data())) return st;
        spans.reserve((size_t)D);
        for (int k = 0; k < D; k++) spans.push_back(span_of(plan[(size_t)k], k, bank, unit));
        const int64_t bad = spans_first_beyond(spans.data(), D, bank.channels, row_units);
        return bad < 0 ? SYLDET_OK : fail(SYLDET_ERR_INVALID_ARGUMENT, "recording " + std::to_string(bad) + " reaches beyond its row");
    }
    // a call's row length on a packed plan is the rows': `name` "n_evals", `of` "evaluations"
    int row_units_arg(int64_t n, const char *name, const char *of) const
    {
        return packed && n != row_units ? packed_rows_refusal(name, std::to_string(row_units) + " " + of) : SYLDET_OK;
    }
    static int packed_rows_refusal(const char *names, const std::string &lengths)
    {
        return fail(SYLDET_ERR_INVALID_ARGUMENT, std::string(names) + " must be the packed rows' " + lengths);
    }
};

// One section of a handle's device block (laid out with carve.hpp's Carver): `bytes` from the host to `at` of the block; a section
// of no bytes copies nothing.
inline hipError_t upload(void *block, size_t at, const void *from, size_t bytes)
{
    return bytes ? hipMemcpy((char *)block + at, from, bytes, hipMemcpyHostToDevice) : hipSuccess;
}
template <class T>
hipError_t upload(void *block, size_t at, const std::vector<T> &from)
{
    return upload(block, at, from.data(), from.size() * sizeof(T));
}
template <class T>
size_t bytes_of(const std::vector<T> &v)
{
    return v.size() * sizeof(T);
}

inline bool engine_known(int32_t e) { return e == SYLDET_ENGINE_AUTO || e == SYLDET_ENGINE_GENERIC || e == SYLDET_ENGINE_FUSED || e == SYLDET_ENGINE_WIDE_BF16; }
// syldet_api.cpp
bool normalised_chain(const syldet_config_t &c);
int64_t count_frames(const syldet *h, int64_t S);
int64_t count_evals(const syldet *h, int64_t S);
bool plan_dft(syldet *h);
bool takes_fold(const syldet_config_t &c, const syldet_geometry_t &g, const syldet::Switches &sw, bool &fused_ok);
int survey_nets(const syldet_config_t *const *cfgs, int32_t n_nets, std::vector<std::unique_ptr<OwnedConfig>> &own, bool &fold, bool &fused_ok);
int choose_engine(syldet *h, int engine);
// syldet_run.cpp (apply_switches: the SYLDET_FUSED_* switches on a plan about to be chosen from or launched, the whole set every time)
void apply_switches(const syldet::Switches &sw, FusedDesc &d);
void forget_call(const syldet *h);    // the handle is going: the thread's last call is not its any more (syldet_last_fused_form)
int run_on_stream(syldet *h, Samples x, int64_t S, int64_t stride, int C, float *d_outputs, uint8_t *d_flags, hipStream_t stream,
                  const int *d_net_of = nullptr, const int *d_row_of = nullptr);
int interleaved_args(const syldet *h, int64_t n_frames, int32_t total_channels);
// syldet_trace.cpp: the [C] fp32 table Float(thresholds[k]) of every channel's own network, on the device (the current one is the handle's)
int trace_thresholds(syldet *h, int k, const float **out);

}  // namespace sd
