// syllable-detector-cli -- the reference's command line tool (SyllableDetectorCLI/main.swift:19-131,
// TrackDetector.swift:45-105) over libsyldet: same options, same output lines
//     channel,sample,seconds,out0[,out1...]
// one per detection event (any output at or above its threshold, TrackDetector.swift:72-77; debounce
// :80,:99), a line with the file name first when more than one file is given (main.swift:122-124).
// All tracks of a file are one batch on the GPU: decode -> H2D -> de-interleave [-> rate conversion when the
// file's rate differs from the network's] -> fused STFT + network kernel -> flags/outputs -> host.
// 16-bit PCM at the network's rate crosses the bus and is de-interleaved as int16 (the library's *_s16 entry points give
// the fp32 path's bits on x / 32768, which is what the decoder would have produced).
// --simulate-dir / --ttl-dir / --ttl-onsets-dir write the same files for any number of audio files; under --batch a batch's tracks are
// made by syldet_recordings_trace_device_s16 / syldet_recordings_trigger*_device_s16 straight into every file's frames.
// --levels-dir writes every file's --levels table likewise; under --batch by syldet_recordings_levels_device* /
// syldet_recordings_output_levels_device on the batch's packed rows.
// --simulate <out.wav> also writes what the reference's Simulator writes (ViewControllerSimulator.swift:251-344): the chosen output
// over its threshold, held between evaluations, as a 16-bit WAV of every track (syldet_trace_interleaved_device_s16).
//
// Differences a user can see: the reference decodes anything AVFoundation can, this tool reads WAV; the
// reference has Core Audio deliver the network's rate (SyllableDetector.swift:19-23), this tool converts the decoded
// file itself: by linear interpolation with fp64 positions (syldet_convert_rate_device; the default) or, with --resample sinc,
// band-limited, which is what Core Audio's delivery is (syldet_convert_rate_sinc_device; a 16-bit file stays int16 up to the
// converter; under --batch such files join the bank and are converted as its rows load, syldet_recordings_load_sinc_device);
// events of different channels are interleaved buffer by buffer like the reference's read loop (main.swift:126-130), with --chunk frames per buffer (AVAssetReader's buffer size is
// not specified; 8192 is what it typically vends for linear PCM).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "syldet.h"
#include "wav.hpp"

namespace {

constexpr int kExUsage = 64;   // EX_USAGE, main.swift:40

void usage(FILE *to)
{
    std::fprintf(to,
                 "Usage: syllable-detector-cli -n <net> [-a <audio>]... [-d <seconds>] [--device <k>] [--chunk <frames>] [--format <shortest|swift4>] [--resample <linear|sinc>] [--resample-quality <Z,beta,rolloff>] [--simulate <out.wav>] [--simulate-output <k>] [--levels <out.tsv>] [--levels-buffer <L>] [--levels-period <seconds>] [--ttl <out.wav>] [--ttl-mux] [--ttl-width <seconds>] [--ttl-steps <n>] [--ttl-buffer <L>] [--ttl-latency <seconds>] [--ttl-onsets <out.tsv>] [--simulate-dir <dir>] [--ttl-dir <dir>] [--ttl-onsets-dir <dir>] [--batch] [--batch-rows <N>] [--batch-bytes <B>] [--score <labels.tsv> --score-out <table.tsv>] [--score-thresholds <lo:hi:n>] [--score-tolerance <seconds>] [--score-cost <c>] [--score-output <k>] [--align-dir <dir>] [--align <columns|outputs|samples>] [--align-at <detections|labels>] [--align-before <units>] [--align-after <units>] [--probe]\n"
                 "  -n, --net <net>:\n      Path to trained network file.  Given k > 1 times: each file must have exactly k tracks, and track t runs network t (one mixed bank; the networks must share the sampling rate, window length, window overlap, time range and number of outputs).\n"
                 "  -a, --audio <audio>:\n      Path to the audio file to process.\n"
                 "  -d, --debounce <seconds>:\n      Number of seconds to debounce triggers.\n"
                 "      --device <k>:\n      HIP device to run on (default 0).\n"
                 "      --chunk <frames>:\n      Frames per decode buffer when interleaving events of several channels (default 8192; 0: channel by channel).\n"
                 "      --format <shortest|swift4>:\n      How numbers are printed: the shortest digits that round-trip (Swift 4.2 and later; default) or 15 / 6 significant digits (Swift 4.0, the toolchain the project declares: the example line below).\n"
                 "      --resample <linear|sinc>:\n      How a file at another sampling rate than the network's is converted: linear interpolation between two neighbours (default) or a band-limited Kaiser-windowed sinc, which filters before it decimates and keeps the band's level.\n"
                 "      --resample-quality <Z,beta,rolloff>:\n      The sinc converter's half width in zero crossings (4 to 64), the Kaiser window's beta (0 to 20) and the cutoff as a fraction of the lower Nyquist frequency (above 0, at most 1); default 32,12,0.9.\n"
                 "      --simulate <out.wav>:\n      Also write the Simulator's output track of every track of the (one) audio file as a 16-bit WAV at the network's sampling rate: the chosen output as a fraction of its threshold (0 = 0, threshold and above = 32767), held from one evaluation to the next.\n"
                 "      --simulate-output <k>:\n      The network output --simulate follows (default 0).\n"
                 "      --levels <out.tsv>:\n      Also write the level meters of every track of the (one) audio file, one line per reading and track, tab separated: the track, the time of the reading's end in seconds, the input RMS (the loudest buffer of the reading), the output level (the greatest first output evaluated in the reading; empty for a reading without an evaluation).\n"
                 "      --levels-dir <dir>:\n      Write what --levels writes for every audio file, as <dir>/<the audio file's name>.tsv, for any number of files; under --batch the readings come from the batch's packed rows in a fixed number of launches, and only the tables come back from the device.\n"
                 "      --levels-buffer <L>:\n      Samples per buffer of the input meter: a power of two from 8 to 4096 (default 32).\n"
                 "      --levels-period <seconds>:\n      Time between two readings (default 0.1); a reading is a whole number of buffers, at least one.\n"
                 "      --ttl <out.wav>:\n      Also write the TTL trigger track of every track of the (one) audio file as a 16-bit WAV at the network's sampling rate: 32767 for the pulse's width from the output buffer behind every input buffer in which a detection became available, 0 elsewhere.\n"
                 "      --ttl-mux:\n      Write --ttl's file with twice the tracks, every audio track followed by its trigger track (16-bit PCM input at the network's rate only).\n"
                 "      --ttl-width <seconds>:\n      Width of a pulse (default 0.001).\n"
                 "      --ttl-steps <n>:\n      Width of a pulse as n buffers (the Arduino output holds for 20), instead of --ttl-width.\n"
                 "      --ttl-buffer <L>:\n      Samples per input and output buffer: a power of two from 8 to 4096 (default 32).\n"
                 "      --ttl-latency <seconds>:\n      Delay of the output behind the input (default 0).\n"
                 "      --ttl-onsets <out.tsv>:\n      Also write the rising edges of the trigger tracks, one line each, tab separated: the track, the sample, the time in seconds.\n"
                 "      --simulate-dir <dir>, --ttl-dir <dir>, --ttl-onsets-dir <dir>:\n      --simulate, --ttl and --ttl-onsets for any number of audio files, with or without --batch: for an audio file p the file written is <dir>/<the file name of p> (the onsets: that name with .tsv behind it), exactly what the option for one file writes for p alone. The directory is made if it is not there; two audio files of the same name are refused. Under --batch a batch's tracks are made on the GPU in one pass and come back in one download per product.\n"
                 "      --batch:\n      Run the audio files through one detector bank instead of one bank a file: every track of every file becomes a recording in the bank's rows, and only the detections come back from the GPU. The output is the same. A file at another sampling rate than the network's joins the bank under --resample sinc (its rate within a sixteenth and sixteen times the network's): it is converted as the rows load, and a batch that holds such a file runs as 32-bit float. Under --resample linear (the default), or outside that range, such a file ends the batch and runs alone, as without --batch.\n"
                 "      --batch-rows <N>:\n      Rows of the bank under --batch (default 64; no more than there are tracks).\n"
                 "      --batch-bytes <B>:\n      Consecutive files share a batch until their samples pass B bytes (default 2147483648); a file that is converted counts with the bytes it has at its own rate. Each track product (--simulate-dir, --ttl-dir) adds 2 bytes per sample at the network's rate to what a batch holds on the device; what --align-dir is cut from counts towards B (see there).\n"
                 "      --score <labels.tsv>:\n      Under --batch, also score every track against labelled times for a grid of candidate thresholds: lines of file, track and sample, tab separated (the file as -a names it, the sample counted from the file's start at the network's sampling rate, also for a file at another rate). A file that does not go through the bank (see --batch) is left out, with a message. Needs --score-out.\n"
                 "      --score-out <table.tsv>:\n      Where --score writes its table, one line per threshold, tab separated: threshold, detections, hits, misses, false positives, repeats, the mean and the standard deviation of the hits' offsets in samples, the cost; a last line names the threshold of the smallest cost.\n"
                 "      --score-thresholds <lo:hi:n>:\n      The grid: n thresholds from lo to hi (default 0:1:101; at most 4096).\n"
                 "      --score-tolerance <seconds>:\n      A detection this close to a label is a hit (default 0.02).\n"
                 "      --score-cost <c>:\n      The cost of a false positive or a repeat; a miss costs 1 (default 1).\n"
                 "      --score-output <k>:\n      The network output --score compares with the thresholds (default 0).\n"
                 "      --align-dir <dir>:\n      Also write, for every audio file p, the windows of a source around every event of every track: <dir>/<the file name of p>.npy (NumPy format 1.0, little-endian float32, shape [events][units][width], all tracks' events in track order; elements outside the track are NaN) and <dir>/<that name>.tsv (one line per window: track, sample, seconds); and behind the last file <dir>/count.npy (int64), <dir>/sum.npy and <dir>/sumsq.npy (float64), shape [networks][units][width]: per position the number of windows that hold it and the sums of their values and squares, one stack per -n network over all files in command-line order. With or without --batch, the same bytes. Under --batch what the windows are cut from counts towards --batch-bytes: 4 + 4 x bins / hop bytes per sample for the columns (4.88 for the example network: the fp32 rows and their columns), 4 for the samples, nothing for the outputs.\n"
                 "      --align <columns|outputs|samples>:\n      What the windows are cut from: the spectrogram's columns (default; a unit is a frame of the band's bins), the network's outputs (a unit is an evaluation) or the samples at the network's rate.\n"
                 "      --align-at <detections|labels>:\n      The events: the detections that are printed (default), or the labelled samples of the file given with --score (which then needs neither --batch nor --score-out).\n"
                 "      --align-before <units>, --align-after <units>:\n      Units of the source in front of and behind the event's own unit (default: the network's time range less one, each; with --align columns --align-before <time range - 1> --align-after 0 a detection's window is the network's input).\n"
                 "      --probe:\n      Only print what the audio files contain; does not touch the GPU.\n"
                 "The command line will write a comma-separated list of detection events (when the network has at least one output above threshold) to standard out. For example, it might output:\n"
                 "\n\t0,1593298,36.1292063492063,0.918557\n\n"
                 "The columns are:\n"
                 "1. The track or channel number from the audio file (starting with 0).\n"
                 "2. The sample number from the audio when detection occurred.\n"
                 "3. The timestamp from the audio when detection occurred.\n"
                 "4. The first neural network output. Note that there may be additional columns for additional outputs.\n");
}

// Swift's description of a Double / Float: the shortest digits that round-trip, with ".0" for whole numbers.
template <typename F>
std::string swift_number(F v)
{
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof buf, v);
    std::string s(buf, r.ptr);
    if (s.find_first_of(".en") == std::string::npos) s += ".0";   // "2" -> "2.0"; leaves "1e+16", "inf", "nan"
    return s;
}

// The same under Swift 4.0 / 4.1, the toolchain the project declares (SWIFT_VERSION = 4.0, project.pbxproj:593): before
// Swift 4.2 `description` printed "%0.*g" with digits10 significant digits -- 15 for Double, 6 for Float -- and appended ".0" when
// the text held neither '.', 'e' nor a letter.  The one output line the reference holds, in its help text (main.swift:33),
// "0,1593298,36.1292063492063,0.918557", is in this form: 15 and 6 digits.
template <typename F>
std::string swift4_number(F v)
{
    char buf[64];
    std::snprintf(buf, sizeof buf, "%0.*g", sizeof(F) == 8 ? 15 : 6, (double)v);
    std::string s(buf);
    if (s.find_first_of(".eEn") == std::string::npos) s += ".0";          // ("inf", "nan" keep their letters)
    return s;
}

bool g_swift4 = false;                                     // --format swift4
template <typename F>
std::string number(F v) { return g_swift4 ? swift4_number(v) : swift_number(v); }

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1) == hipSuccess; }
};

struct Event { int64_t buffer; int channel; int64_t sample; int64_t eval; };

// --levels: the two meters of every row (Processor.swift:111-113, :138, :158-184) over the recording, as the 0.1 s timer of
// ViewControllerProcessor.swift:57 would have read them
struct LevelsOpt {
    std::string path;                                      // empty: none
    int buffer = 32;                                       // AudioInterface.swift:342, :474
    double period = 0.1;
};

// --ttl / --ttl-onsets: the pulses the rig would have emitted (Processor.swift:128-148, AudioInterface.swift:13-40, :442-445)
struct TtlOpt {
    std::string path, onsets;                              // empty: none
    bool mux = false;
    double width = 0.001, latency = 0.0;                   // ProcessorAudio :217-221
    long steps = 0;                                        // > 0: the width as buffers (ProcessorArduino :266-291 holds for 20)
    int buffer = 32;
    bool any() const { return !path.empty() || !onsets.empty(); }
    int64_t width_samples(double rate) const { return steps > 0 ? (int64_t)steps * buffer : syldet_trigger_width(width, rate); }
    int64_t latency_samples(double rate) const { const double x = latency * rate; return x < 9e18 ? (int64_t)x : INT64_MAX; }
};

// --simulate-dir / --ttl-dir / --ttl-onsets-dir: the per-sample products of every audio file, each under its file's name
struct TrackDirs {
    std::string simulate, ttl, onsets;                     // empty: none
    std::string levels;                                    // --levels-dir: every file's level table, <name>.tsv (not a track: any() leaves it out)
    bool any() const { return !simulate.empty() || !ttl.empty() || !onsets.empty(); }
    static std::string name_of(const std::string &path)
    {
        const size_t at = path.find_last_of('/');
        return at == std::string::npos ? path : path.substr(at + 1);
    }
    static std::string in(const std::string &dir, const std::string &path, const char *suffix = "")
    {
        return dir.empty() ? std::string() : dir + "/" + name_of(path) + suffix;
    }
    // what process_file takes for one audio file
    std::string simulate_for(const std::string &path, const std::string &single) const { return simulate.empty() ? single : in(simulate, path); }
    template <class Ttl>
    Ttl ttl_for(const std::string &path, Ttl t) const
    {
        if (!ttl.empty()) t.path = in(ttl, path);
        if (!onsets.empty()) t.onsets = in(onsets, path, ".tsv");
        return t;
    }
    template <class Levels>
    Levels levels_for(const std::string &path, Levels l) const
    {
        if (!levels.empty()) l.path = in(levels, path, ".tsv");
        return l;
    }
    void make() const                                      // (a directory that cannot be made: the writes fail, and cost what they cost)
    {
        std::error_code ec;
        for (const std::string *d : {&simulate, &ttl, &onsets, &levels})
            if (!d->empty()) std::filesystem::create_directories(*d, ec);
    }
};

// the rising edges as --ttl-onsets writes them: track, sample, seconds
bool write_onsets(const std::string &path, int C, const int64_t *idx, const int64_t *cnt, int64_t cap, double rate);

// --resample / --resample-quality: how a file at another rate is brought to the network's (the step the reference's tool leaves to
// AVFoundation, SyllableDetector.swift:19-23, TrackDetector.swift:35)
struct ResampleOpt {
    bool sinc = false;                                     // false: syldet_convert_rate_device
    int32_t zero_crossings = 0;                            // syldet_sinc_defaults unless --resample-quality
    double beta = 0.0, rolloff = 0.0;
};

// --align-dir: event-aligned windows (syldet_aligner_*, syldet_align_device): for every audio file the units of a source around
// every detection (or label) of every track, one window an event, as <dir>/<name>.npy with <name>.tsv beside it; and, over all files
// in command-line order, the stack statistics of every network's events as <dir>/count.npy, sum.npy and sumsq.npy.  The stacks are
// added on the host in the library's tree (blocks of SYLDET_ALIGN_BLOCK events through syldet_align_stats_host, the blocks in
// order), fed file by file, so that they do not depend on how the files were batched.
struct AlignOpt {
    std::string dir;                                       // empty: none
    int source = SYLDET_ALIGN_COLUMNS;
    bool at_labels = false;
    long before = -1, after = -1;                          // < 0: timeRange - 1
};

struct AlignRun {
    AlignOpt opt;
    const std::map<std::string, std::map<long, std::vector<int64_t>>> *labels = nullptr;   // --align-at labels: --score's file
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
AlignRun *g_align = nullptr;                               // --align-dir was given

// NumPy format 1.0, little endian, C order
bool write_npy(const std::string &path, const char *descr, const std::vector<int64_t> &shape, const void *data, size_t bytes)
{
    std::string dict = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': (";
    for (size_t i = 0; i < shape.size(); i++) dict += std::to_string(shape[i]) + (shape.size() == 1 || i + 1 < shape.size() ? "," : "") + (i + 1 < shape.size() ? " " : "");
    dict += "), }";
    while ((10 + dict.size() + 1) % 64 != 0) dict += ' ';
    dict += '\n';
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const unsigned char head[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (unsigned char)(dict.size() & 255), (unsigned char)(dict.size() >> 8)};
    bool ok = std::fwrite(head, 1, 10, f) == 10 && std::fwrite(dict.data(), 1, dict.size(), f) == dict.size() && (bytes == 0 || std::fwrite(data, 1, bytes, f) == bytes);
    if (std::fclose(f) != 0) ok = false;
    return ok;
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

// The windows of one bank's detectors -- a batch's recordings (r), or a file's tracks (r NULL) -- in one launch, and back: windows
// [N][n][width] with detector d's events from begin[d].  d_src: the source on the device, n_units units a row.
bool align_windows(AlignRun &run, syldet_t *h, syldet_recordings_t *r, const float *d_src, int64_t n_units, int64_t row_stride,
                   const std::vector<std::vector<int64_t>> &events, hipStream_t stream, std::vector<float> &windows, std::vector<int64_t> &begin)
{
    begin.assign(1, 0);
    std::vector<int64_t> flat;
    for (const std::vector<int64_t> &e : events) {
        flat.insert(flat.end(), e.begin(), e.end());
        begin.push_back((int64_t)flat.size());
    }
    const int64_t N = begin.back();
    windows.assign((size_t)N * (size_t)run.L(), 0.0f);
    syldet_aligner_t *a = nullptr;
    int st = syldet_aligner_create(h, r, run.opt.source, run.before, run.after, &a);
    DevBuf d_events, d_windows;
    bool ok = true;
    if (!st && N > 0) {
        ok = d_events.alloc(flat.size() * sizeof(int64_t)) && d_windows.alloc(windows.size() * sizeof(float)) &&
             hipMemcpyAsync(d_events.p, flat.data(), flat.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream) == hipSuccess;
        if (ok) st = syldet_align_device(a, d_src, n_units, row_stride, (const int64_t *)d_events.p, 0, begin.data(), std::nanf(""), (float *)d_windows.p, stream);
        if (ok && !st) ok = hipMemcpyAsync(windows.data(), d_windows.p, windows.size() * sizeof(float), hipMemcpyDeviceToHost, stream) == hipSuccess;
    }
    if (ok && hipStreamSynchronize(stream) != hipSuccess) ok = false;
    syldet_aligner_destroy(a);
    if (st) std::fprintf(stderr, "Unable to align the events: %s: %s\n", syldet_strerror(st), syldet_last_error());
    return ok && st == 0;
}

// One audio file's windows and their table, and its events into the networks' stacks: track by track, event by event.  units[t]:
// the units of the source that track t has (what decides which elements of a window are present).  0, or 3: a file is not written.
int align_write_file(AlignRun &run, const std::string &path, const std::vector<std::vector<int64_t>> &events, const std::vector<int64_t> &units,
                     const float *windows, int64_t origin, int64_t step, double rate)
{
    const int64_t L = run.L();
    int64_t N = 0;
    for (const std::vector<int64_t> &e : events) N += (int64_t)e.size();
    const std::string npy = TrackDirs::in(run.opt.dir, path, ".npy"), tsv = TrackDirs::in(run.opt.dir, path, ".tsv");
    int bad = 0;
    if (!write_npy(npy, "<f4", {N, run.n, (int64_t)run.width}, windows, (size_t)N * (size_t)L * sizeof(float))) {
        std::fprintf(stderr, "Unable to write %s.\n", npy.c_str());
        bad = 3;
    }
    FILE *f = std::fopen(tsv.c_str(), "w");
    bool ok = f != nullptr;
    int64_t w = 0;
    for (size_t t = 0; t < events.size(); t++) {
        AlignRun::Stack &st = run.stacks[run.networks > 1 ? t % (size_t)run.networks : 0];
        for (const int64_t s : events[t]) {
            if (ok) ok = std::fputs((std::to_string(t) + "\t" + std::to_string(s) + "\t" + number((double)s / rate) + "\n").c_str(), f) >= 0;
            // the present elements of the window: the units u0 - before .. u0 + after that lie in [0, units) (include/syldet.h)
            const int64_t c = s < -(((int64_t)1 << 62) - 1) ? -(((int64_t)1 << 62) - 1) : s > ((int64_t)1 << 62) - 1 ? ((int64_t)1 << 62) - 1 : s;
            int64_t u0 = (c - origin) / step;
            if (u0 * step > c - origin) u0--;                // a floor, also for a negative numerator
            const int64_t lo = u0 - run.before, first = std::max<int64_t>(lo, 0), last = std::min<int64_t>(u0 + run.after, units[t] - 1);
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
        if (!write_npy(path, i == 0 ? "<i8" : "<f8", shape, data, L * run.stacks.size() * 8)) {
            std::fprintf(stderr, "Unable to write %s.\n", path.c_str());
            ok = false;
        }
    }
    return ok;
}

// the events --align-at names for one track of one file: its labels (--score's file), or the detections given
std::vector<int64_t> align_events_of(const AlignRun &run, const std::string &path, int track, const std::vector<int64_t> &detections)
{
    if (!run.opt.at_labels) return detections;
    const auto of_file = run.labels->find(path);
    if (of_file == run.labels->end()) return {};
    const auto of_track = of_file->second.find(track);
    return of_track == of_file->second.end() ? std::vector<int64_t>() : of_track->second;
}

// cfgs: one network for every track, or (k > 1) network t for track t of a file of exactly k tracks, through one mixed bank
// (syldet_create_mixed): the networks share the evaluation clock, so the events are found and printed as for one
// simulate: a path for the Simulator's output track (ViewControllerSimulator.swift:251-344) of every track, made on the device from
// the outputs the run left there (syldet_trace_interleaved_device_s16) and written as a 16-bit WAV of as many frames as the detector
// was fed, at the network's rate; empty: none
int process_file(const std::string &path, const std::vector<syldet_config_t *> &cfgs, int device, double debounce_s, bool have_debounce, int64_t chunk,
                 const std::string &simulate = std::string(), int simulate_output = 0, const LevelsOpt &levels = LevelsOpt(),
                 const TtlOpt &ttl = TtlOpt(), const ResampleOpt &conv = ResampleOpt())
{
    const syldet_config_t *cfg = cfgs[0];
    wav::Info info;
    std::vector<float> frames;
    std::vector<int16_t> frames16;
    std::string err;
    // 16-bit PCM at the network's rate goes to the device as stored (syldet_run_interleaved_device_s16: the fp32 call's results
    // on x / 32768, half the bytes); any other file is decoded to fp32 here
    const bool file16 = wav::probe(path, info, err) && info.format == 1 && info.bits == 16;
    const bool pcm16 = file16 && info.rate == cfgs[0]->sampling_rate;
    // ... and so does 16-bit PCM at another rate on its way to the band-limited converter, which reads int16 rows itself
    const bool raw16 = pcm16 || (file16 && conv.sinc);
    err.clear();
    if (raw16 ? !wav::read_s16(path, info, frames16, err) : !wav::read(path, info, frames, err)) {
        std::fprintf(stderr, "Unable to read %s: %s\n", path.c_str(), err.c_str());
        return 1;
    }
    const int C = info.channels;
    if (C <= 0 || info.frames <= 0) {
        std::fprintf(stderr, "No audio tracks found in %s.\n", path.c_str());
        return 1;
    }
    // (like a track that cannot be written, this does not cost the detection lines)
    const bool mux_refused = ttl.mux && !pcm16;
    if (mux_refused) std::fprintf(stderr, "Unable to write %s: --ttl-mux takes 16-bit PCM at the network's sampling rate (%s).\n", ttl.path.c_str(), path.c_str());
    if (cfgs.size() > 1 && (size_t)C != cfgs.size()) {
        std::fprintf(stderr, "Unable to process %s: it has %d track(s), but %zu networks were given (one per track).\n", path.c_str(), C, cfgs.size());
        return 1;
    }
    syldet_t *h = nullptr;
    std::vector<int32_t> track_net((size_t)C);
    for (int t = 0; t < C; t++) track_net[(size_t)t] = t;
    if (int st = cfgs.size() > 1 ? syldet_create_mixed(cfgs.data(), (int32_t)cfgs.size(), track_net.data(), C, device, SYLDET_ENGINE_AUTO, &h)
                                 : syldet_create(cfg, C, device, SYLDET_ENGINE_AUTO, &h)) {
        std::fprintf(stderr, "Unable to create the detector: %s: %s\n", syldet_strerror(st), syldet_last_error());
        return 2;
    }
    syldet_geometry_t g;
    syldet_get_geometry(h, &g);
    const int n_out = g.outputs;
    const bool resample = info.rate != cfg->sampling_rate;
    int rc = 0;
    hipStream_t stream = nullptr;
    std::vector<float> out;
    std::vector<uint8_t> flags;
    std::vector<int16_t> track;
    std::vector<double> lv_in;                              // [C][M] mean squares
    std::vector<float> lv_out;                              // [C][M]
    std::vector<uint8_t> lv_empty;                          // [M] the reading holds no evaluation
    std::vector<int16_t> ttl_track;                         // [S][C] or (--ttl-mux) [S][2 C]
    std::vector<int64_t> ttl_idx, ttl_cnt;                  // [C][ttl_cap], [C]
    int64_t ttl_cap = 1;
    int64_t lv_P = 1, lv_M = 0;
    int64_t E = 0, fed = 0;
    // --align-dir: every track's events, their windows, and what decides presence
    std::vector<std::vector<int64_t>> al_events;
    std::vector<int64_t> al_units, al_begin;
    std::vector<float> al_windows;
    int64_t al_origin = 0, al_step = 1;
    bool al_made = false;
    const int64_t debounce_of_file = have_debounce ? (int64_t)(debounce_s * cfg->sampling_rate) : 0;   // Int(newValue * samplingRate), TrackDetector.swift:24
    do {
        if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&stream) != hipSuccess) { rc = 2; break; }
        const int64_t n = info.frames;
        DevBuf d_inter, d_planar, d_res, d_out, d_flags;
        const size_t in_bytes = (size_t)n * C * (raw16 ? sizeof(int16_t) : sizeof(float));
        if (!d_inter.alloc(in_bytes)) { rc = 2; break; }
        if (hipMemcpyAsync(d_inter.p, raw16 ? (const void *)frames16.data() : (const void *)frames.data(), in_bytes, hipMemcpyHostToDevice, stream) != hipSuccess) { rc = 2; break; }
        int64_t S = n, res_stride = 0;
        int st = 0;
        if (resample) {
            // The reference's tool has AVFoundation deliver every track at the network's rate (SyllableDetector.swift:19-23,
            // TrackDetector.swift:35); here: linear interpolation of the whole decoded file with fp64 positions
            // (syldet_convert_rate_device; ResamplerLinear is the live path's streaming object, not a file converter) or, with
            // --resample sinc, the band-limited converter -- on the int16 rows of a 16-bit file, which never become fp32 input
            res_stride = syldet_convert_rate_count(n, info.rate, cfg->sampling_rate);
            if (!d_planar.alloc((size_t)C * n * (raw16 ? sizeof(int16_t) : sizeof(float))) || !d_res.alloc((size_t)C * (res_stride > 0 ? res_stride : 1) * sizeof(float))) { rc = 2; break; }
            if (raw16) {
                st = syldet_deinterleave_device_s16((const int16_t *)d_inter.p, n, C, C, (int16_t *)d_planar.p, n, stream);
                if (!st) st = syldet_convert_rate_sinc_device_s16((const int16_t *)d_planar.p, n, n, C, info.rate, cfg->sampling_rate, conv.zero_crossings, conv.beta, conv.rolloff, (float *)d_res.p, res_stride, &S, stream);
            } else {
                st = syldet_deinterleave_device((const float *)d_inter.p, n, C, 0, C, (float *)d_planar.p, n, stream);
                if (!st && conv.sinc) st = syldet_convert_rate_sinc_device((const float *)d_planar.p, n, n, C, info.rate, cfg->sampling_rate, conv.zero_crossings, conv.beta, conv.rolloff, (float *)d_res.p, res_stride, &S, stream);
                else if (!st) st = syldet_convert_rate_device((const float *)d_planar.p, n, n, C, info.rate, cfg->sampling_rate, (float *)d_res.p, res_stride, &S, stream);
            }
            if (st) {
                std::fprintf(stderr, "Unable to process %s: %s: %s\n", path.c_str(), syldet_strerror(st), syldet_last_error());
                rc = 2;
                break;
            }
        }
        E = syldet_count_evals(h, S);
        fed = S;
        DevBuf d_track, d_lv_in, d_lv_out;
        if (E <= 0 && !simulate.empty()) track.assign((size_t)S * C, 0);   // shorter than one evaluation: a track of zeros
        // the meters: the input readings of the samples the detector is fed (queued here, behind the copy; a recording shorter
        // than one evaluation has them too), the output readings behind the run
        auto meters = [&](bool outputs_too) -> bool {
            if (levels.path.empty() || S <= 0) return true;
            const double per = levels.period * cfg->sampling_rate / (double)levels.buffer;
            lv_P = per >= 1.0 ? (per < 9e18 ? (int64_t)per : INT64_MAX) : 1;
            lv_M = syldet_levels_count(S, levels.buffer, lv_P);
            const size_t cells = (size_t)C * (size_t)lv_M;
            if (!outputs_too) {
                lv_in.resize(cells);
                if (!d_lv_in.alloc(cells * sizeof(double))) return false;
                if (pcm16) st = syldet_levels_interleaved_device_s16(h, (const int16_t *)d_inter.p, n, C, levels.buffer, lv_P, (double *)d_lv_in.p, stream);
                else if (!resample) st = syldet_levels_interleaved_device(h, (const float *)d_inter.p, n, C, levels.buffer, lv_P, (double *)d_lv_in.p, stream);
                else st = syldet_levels_device(h, (const float *)d_res.p, S, res_stride, levels.buffer, lv_P, (double *)d_lv_in.p, stream);
                if (!st && hipMemcpyAsync(lv_in.data(), d_lv_in.p, cells * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess) return false;
            } else {
                lv_out.resize(cells);
                if (!d_lv_out.alloc(cells * sizeof(float))) return false;
                st = syldet_output_levels_device(h, (const float *)d_out.p, E, 0, S, levels.buffer, lv_P, (float *)d_lv_out.p, stream);
                if (!st && hipMemcpyAsync(lv_out.data(), d_lv_out.p, cells * sizeof(float), hipMemcpyDeviceToHost, stream) != hipSuccess) return false;
            }
            if (st) std::fprintf(stderr, "Unable to meter %s: %s: %s\n", path.c_str(), syldet_strerror(st), syldet_last_error());
            return st == 0;
        };
        if (!meters(false)) { rc = 2; break; }
        // the trigger tracks and their rising edges from the flags the run left on the device (no evaluation: no flag, zeros)
        DevBuf d_ttl, d_ttl_idx, d_ttl_cnt, d_rows;
        auto triggers = [&]() -> bool {
            if (!ttl.any() || S <= 0) return true;
            const int64_t N = ttl.width_samples(cfg->sampling_rate), lat = ttl.latency_samples(cfg->sampling_rate), nE = E > 0 ? E : 0;
            if (!d_flags.p && !d_flags.alloc(1)) return false;
            if (!ttl.path.empty() && !mux_refused) {
                ttl_track.resize((size_t)S * C * (ttl.mux ? 2 : 1));
                if (!d_ttl.alloc(ttl_track.size() * sizeof(int16_t))) return false;
                if (ttl.mux) {
                    // the recording as planar int16 rows, the layout syldet_run_device_s16 takes: from the frames already on the device
                    if (!d_rows.alloc((size_t)C * S * sizeof(int16_t))) return false;
                    st = syldet_deinterleave_device_s16((const int16_t *)d_inter.p, S, C, C, (int16_t *)d_rows.p, S, stream);
                    if (!st) st = syldet_trigger_mux_device_s16(h, (const uint8_t *)d_flags.p, nE, ttl.buffer, N, lat, (const int16_t *)d_rows.p, S, (int16_t *)d_ttl.p, S, stream);
                } else {
                    st = syldet_trigger_interleaved_device_s16(h, (const uint8_t *)d_flags.p, nE, ttl.buffer, N, lat, (int16_t *)d_ttl.p, S, stream);
                }
                if (!st && hipMemcpyAsync(ttl_track.data(), d_ttl.p, ttl_track.size() * sizeof(int16_t), hipMemcpyDeviceToHost, stream) != hipSuccess) return false;
            }
            if (!st && !ttl.onsets.empty()) {
                ttl_cap = std::max<int64_t>(1, std::min<int64_t>(nE, S / ttl.buffer + 1));
                ttl_idx.assign((size_t)C * (size_t)ttl_cap, 0);
                ttl_cnt.assign((size_t)C, 0);
                if (!d_ttl_idx.alloc(ttl_idx.size() * sizeof(int64_t)) || !d_ttl_cnt.alloc(ttl_cnt.size() * sizeof(int64_t))) return false;
                st = syldet_trigger_onsets_device(h, (const uint8_t *)d_flags.p, nE, ttl.buffer, N, lat, S, (int64_t *)d_ttl_idx.p, ttl_cap, (int64_t *)d_ttl_cnt.p, stream);
                if (!st && (hipMemcpyAsync(ttl_idx.data(), d_ttl_idx.p, ttl_idx.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
                            hipMemcpyAsync(ttl_cnt.data(), d_ttl_cnt.p, ttl_cnt.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream) != hipSuccess)) return false;
            }
            if (st) std::fprintf(stderr, "Unable to make the trigger track of %s: %s: %s\n", path.c_str(), syldet_strerror(st), syldet_last_error());
            return st == 0;
        };
        // the windows of every track's events (--align-dir), from arrays on the device: the outputs the run left, the fp32 rows the
        // detector was fed, or their columns (syldet_spectrogram_device).  Behind the download of the flags: the detections are made
        // from them as below.
        DevBuf d_al_rows, d_al_cols;
        auto aligned = [&]() -> bool {
            if (!g_align) return true;
            AlignRun &run = *g_align;
            if (syldet_align_anchor(h, run.opt.source, &al_origin, &al_step, nullptr)) {
                std::fprintf(stderr, "Unable to align the events of %s: %s: %s\n", path.c_str(), syldet_strerror(SYLDET_ERR_UNSUPPORTED), syldet_last_error());
                return true;                                // (no files for it: write_files reports them)
            }
            al_events.assign((size_t)C, std::vector<int64_t>());
            for (int c = 0; c < C; c++) {
                std::vector<int64_t> found;
                int64_t until = -1;
                for (int64_t e = 0; !run.opt.at_labels && e < E; e++) {
                    const int64_t idx = (int64_t)g.first_index + e * (int64_t)g.hop;
                    if (!flags[(size_t)c * E + e] || !(until < idx)) continue;
                    until = idx + debounce_of_file;
                    found.push_back(idx);
                }
                al_events[(size_t)c] = align_events_of(run, path, c, found);
            }
            const float *rows = nullptr, *src = nullptr;
            int64_t stride = S, n_units = 0, row_stride = 0;
            if (run.opt.source != SYLDET_ALIGN_OUTPUTS) {
                if (resample) {
                    rows = (const float *)d_res.p;
                    stride = res_stride;
                } else {
                    // the file's tracks as fp32 rows: what the detector was fed (16-bit PCM: x * 2^-15, exact)
                    std::vector<float> planar((size_t)C * (size_t)S);
                    for (int64_t i = 0; i < S; i++)
                        for (int c = 0; c < C; c++)
                            planar[(size_t)c * (size_t)S + (size_t)i] = raw16 ? (float)frames16[(size_t)i * C + c] * (1.0f / 32768.0f) : frames[(size_t)i * C + c];
                    if (!d_al_rows.alloc(planar.size() * sizeof(float)) || hipMemcpy(d_al_rows.p, planar.data(), planar.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return false;
                    rows = (const float *)d_al_rows.p;
                }
            }
            const int64_t J = std::max<int64_t>(0, syldet_count_frames(h, S));
            if (run.opt.source == SYLDET_ALIGN_SAMPLES) {
                src = rows;
                n_units = S;
                row_stride = stride;
            } else if (run.opt.source == SYLDET_ALIGN_COLUMNS) {
                if (!d_al_cols.alloc((size_t)C * (size_t)J * (size_t)run.width * sizeof(float))) return false;
                if (J > 0) st = syldet_spectrogram_device(h, rows, S, stride, (float *)d_al_cols.p, stream);
                if (st) {
                    std::fprintf(stderr, "Unable to align the events of %s: %s: %s\n", path.c_str(), syldet_strerror(st), syldet_last_error());
                    return false;
                }
                src = (const float *)d_al_cols.p;
                n_units = J;
            } else {
                src = (const float *)d_out.p;
                n_units = E > 0 ? E : 0;
            }
            al_units.assign((size_t)C, n_units);
            al_made = align_windows(run, h, nullptr, src, n_units, row_stride, al_events, stream, al_windows, al_begin);
            return al_made;
        };
        if (E <= 0) {                                       // shorter than one evaluation: no events
            if (!triggers()) { rc = 2; break; }
            if ((!levels.path.empty() || ttl.any()) && hipStreamSynchronize(stream) != hipSuccess) rc = 2;
            if (!rc) (void)aligned();                      // (windows that cannot be made do not cost the lines: write_files reports them)
            break;
        }
        if (!d_out.alloc((size_t)C * E * n_out * sizeof(float)) || !d_flags.alloc((size_t)C * E)) { rc = 2; break; }
        if (pcm16) st = syldet_run_interleaved_device_s16(h, (const int16_t *)d_inter.p, n, C, (float *)d_out.p, (uint8_t *)d_flags.p, stream);
        else if (!resample) st = syldet_run_interleaved_device(h, (const float *)d_inter.p, n, C, (float *)d_out.p, (uint8_t *)d_flags.p, stream);
        else st = syldet_run_device(h, (const float *)d_res.p, S, res_stride, (float *)d_out.p, (uint8_t *)d_flags.p, stream);
        if (st) {
            std::fprintf(stderr, "Unable to process %s: %s: %s\n", path.c_str(), syldet_strerror(st), syldet_last_error());
            rc = 2;
            break;
        }
        if (!simulate.empty()) {
            track.resize((size_t)S * C);
            if (!d_track.alloc(track.size() * sizeof(int16_t))) { rc = 2; break; }
            st = syldet_trace_interleaved_device_s16(h, (const float *)d_out.p, E, simulate_output, (int16_t *)d_track.p, S, stream);
            if (st) {
                std::fprintf(stderr, "Unable to simulate %s: %s: %s\n", path.c_str(), syldet_strerror(st), syldet_last_error());
                rc = 2;
                break;
            }
            if (hipMemcpyAsync(track.data(), d_track.p, track.size() * sizeof(int16_t), hipMemcpyDeviceToHost, stream) != hipSuccess) { rc = 2; break; }
        }
        if (!meters(true)) { rc = 2; break; }
        if (!triggers()) { rc = 2; break; }
        out.resize((size_t)C * E * n_out);
        flags.resize((size_t)C * E);
        if (hipMemcpyAsync(out.data(), d_out.p, out.size() * sizeof(float), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipMemcpyAsync(flags.data(), d_flags.p, flags.size(), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) { rc = 2; break; }
        (void)aligned();
    } while (false);
    if (rc == 2 && hipPeekAtLastError() != hipSuccess) std::fprintf(stderr, "Unable to process %s: %s\n", path.c_str(), hipGetErrorString(hipGetLastError()));
    if (stream) (void)hipStreamDestroy(stream);
    if (!rc && !levels.path.empty()) {
        lv_empty.assign((size_t)lv_M, 1);
        for (int64_t m = 0; m < lv_M; m++) {
            int64_t first = 0, count = 0;
            if (syldet_levels_eval_range(h, fed, E > 0 ? E : 0, levels.buffer, lv_P, m, &first, &count) == SYLDET_OK) lv_empty[(size_t)m] = count == 0;
        }
    }
    syldet_destroy(h);
    // the track is written behind the detection lines, which a failing write must not cost: 3 = the lines are out, the track is not
    auto write_track = [&]() -> int {
        if (simulate.empty()) return 0;
        std::string werr;
        if (wav::write_s16(simulate, cfg->sampling_rate, C, fed, track.data(), werr)) return 0;
        std::fprintf(stderr, "Unable to write %s: %s\n", simulate.c_str(), werr.c_str());
        return 3;
    };
    // ... and so are the meters' readings: track, time of the reading's end, input RMS, output level (empty: no evaluation)
    auto write_levels = [&]() -> int {
        if (levels.path.empty()) return 0;
        FILE *f = std::fopen(levels.path.c_str(), "w");
        bool ok = f != nullptr;
        const int64_t PL = std::min(lv_P, (fed + levels.buffer - 1) / levels.buffer) * levels.buffer;
        for (int64_t m = 0; ok && m < lv_M; m++)
            for (int c = 0; ok && c < C; c++) {
                const size_t at = (size_t)c * (size_t)lv_M + (size_t)m;
                const std::string line = std::to_string(c) + "\t" + number((double)std::min((m + 1) * PL, fed) / cfg->sampling_rate) + "\t" +
                                         number(std::sqrt(lv_in[at])) + "\t" + (lv_empty[(size_t)m] ? std::string() : number(lv_out[at])) + "\n";
                ok = std::fputs(line.c_str(), f) >= 0;
            }
        if (f && std::fclose(f) != 0) ok = false;
        if (ok) return 0;
        std::fprintf(stderr, "Unable to write %s.\n", levels.path.c_str());
        return 3;
    };
    // ... and the trigger tracks and their rising edges: track, sample, seconds
    auto write_ttl = [&]() -> int {
        int bad = mux_refused ? 3 : 0;
        if (!ttl.path.empty() && !mux_refused) {
            std::string werr;
            if (!wav::write_s16(ttl.path, cfg->sampling_rate, ttl.mux ? 2 * C : C, fed, ttl_track.data(), werr)) {
                std::fprintf(stderr, "Unable to write %s: %s\n", ttl.path.c_str(), werr.c_str());
                bad = 3;
            }
        }
        if (!ttl.onsets.empty()) {
            if (!write_onsets(ttl.onsets, ttl_cnt.empty() ? 0 : C, ttl_idx.data(), ttl_cnt.data(), ttl_cap, cfg->sampling_rate)) {
                std::fprintf(stderr, "Unable to write %s.\n", ttl.onsets.c_str());
                bad = 3;
            }
        }
        return bad;
    };
    // ... and the windows at the events, with their table (and the events into the stacks)
    auto write_aligned = [&]() -> int {
        if (!g_align) return 0;
        if (!al_made) return 3;
        return align_write_file(*g_align, path, al_events, al_units, al_windows.data(), al_origin, al_step, cfg->sampling_rate);
    };
    auto write_files = [&]() -> int {
        const int a = write_track(), b = write_levels(), c = write_ttl(), d = write_aligned();
        return a ? a : (b ? b : (c ? c : d));
    };
    if (rc) return rc;
    if (E <= 0) return write_files();

    // events: sample number of evaluation e = first_index + e*hop (TrackDetector.swift:39-43,67-68); debounce :80,:99
    const int64_t debounce_frames = debounce_of_file;
    std::vector<Event> events;
    for (int c = 0; c < C; c++) {
        int64_t until = -1;
        for (int64_t e = 0; e < E; e++) {
            if (!flags[(size_t)c * E + e]) continue;
            const int64_t idx = (int64_t)g.first_index + e * (int64_t)g.hop;
            if (!(until < idx)) continue;
            until = idx + debounce_frames;
            events.push_back({chunk > 0 ? (idx - 1) / chunk : 0, c, idx, e});
        }
    }
    // the reference's loop hands every track one buffer per round (main.swift:126-130)
    std::stable_sort(events.begin(), events.end(), [](const Event &a, const Event &b) {
        if (a.buffer != b.buffer) return a.buffer < b.buffer;
        if (a.channel != b.channel) return a.channel < b.channel;
        return a.sample < b.sample;
    });
    for (const Event &ev : events) {
        std::string line = std::to_string(ev.channel) + "," + std::to_string(ev.sample) + "," +
                           number((double)ev.sample / cfg->sampling_rate);
        for (int o = 0; o < n_out; o++) line += "," + number(out[((size_t)ev.channel * E + ev.eval) * n_out + o]);
        std::puts(line.c_str());
    }
    std::fflush(stdout);
    return write_files();
}

bool write_onsets(const std::string &path, int C, const int64_t *idx, const int64_t *cnt, int64_t cap, double rate)
{
    FILE *f = std::fopen(path.c_str(), "w");
    bool ok = f != nullptr;
    for (int c = 0; ok && c < C; c++)
        for (int64_t i = 0; ok && i < std::min(cnt[(size_t)c], cap); i++) {
            const int64_t smp = idx[(size_t)c * (size_t)cap + (size_t)i];
            const std::string line = std::to_string(c) + "\t" + std::to_string(smp) + "\t" + number((double)smp / rate) + "\n";
            ok = std::fputs(line.c_str(), f) >= 0;
        }
    if (f && std::fclose(f) != 0) ok = false;
    return ok;
}

// --batch: the -a files through ONE bank instead of a bank a file (syldet_recordings_*: every track of every file of a batch is a
// recording laid into the bank's rows; the reference's tool runs them one after another on one core, main.swift:63-130).  Only
// the detections and their outputs come back from the device -- and, under --simulate-dir / --ttl-dir / --ttl-onsets-dir, every
// file's tracks: one device buffer a product, every file's frame-major int16 frames [n][tracks] end to end, each file from a multiple
// of 8 elements, written by ONE call a product (step = the file's track count, offset = the file's base + the track) and brought
// back in one download.  What is printed is what the loop over process_file prints.
struct BatchOpt {
    bool on = false;
    long rows = 64;
    long long bytes = 2ll << 30;
};

struct BatchFile {
    std::string path;
    wav::Info info;
    std::vector<unsigned char> raw;                         // the frames as the file's data chunk stores them (wav::read_raw)
    bool is16 = false;
    bool convert = false;                                   // at another rate than the network's: converted as the rows load (--resample sinc)
    // what --batch counts: the bytes of the rows the file's samples make at its own rate (int16 rows for a 16-bit file, else fp32)
    size_t bytes() const { return (size_t)info.frames * (size_t)info.channels * (is16 ? sizeof(int16_t) : sizeof(float)); }
    int sample_bytes() const { return info.bits / 8; }
    int32_t format() const                                  // SYLDET_PCM_* of the file's samples
    {
        if (info.format == 3) return info.bits == 32 ? SYLDET_PCM_F32 : SYLDET_PCM_F64;
        return info.bits == 8 ? SYLDET_PCM_U8 : info.bits == 16 ? SYLDET_PCM_S16 : info.bits == 24 ? SYLDET_PCM_S24 : SYLDET_PCM_S32;
    }
};

// --score: threshold calibration (syldet_scorer_*): every track of every batched file scored against its labelled samples for
// a grid of candidate thresholds, on the outputs the batch leaves on the device.  The batches' tables add up on the host.
struct ScoreOpt {
    std::string labels_path, out_path;
    double lo = 0.0, hi = 1.0, tolerance = 0.02, cost = 1.0;
    long n = 101;
    int output = 0;
    bool on() const { return !labels_path.empty(); }
};

struct ScoreRun {
    std::vector<double> thresholds;
    int output = 0;
    int64_t tolerance = 0;                                  // samples
    std::map<std::string, std::map<long, std::vector<int64_t>>> labels;   // file as -a names it -> track -> sorted samples
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

// One batch: returns 0, 2 for device trouble (no line of the batch is printed then, but the files' names are), or 3: the lines are
// out, a track is not
int run_batch(std::vector<BatchFile> &files, const std::vector<syldet_config_t *> &cfgs, int device, double debounce_s, int64_t chunk,
              long max_rows, bool headers, ScoreRun *score, const ResampleOpt &conv, const TrackDirs &dirs, int simulate_output, const TtlOpt &ttl,
              const LevelsOpt &levels)
{
    if (files.empty()) return 0;
    const syldet_config_t *cfg = cfgs[0];
    bool all16 = true, converting = false;
    for (const BatchFile &f : files) {
        all16 = all16 && f.is16;
        converting = converting || f.convert;
    }
    // a batch that holds a file at another rate: every recording is planned with its length at the network's rate and loaded
    // through the converting load (syldet_recordings_load_sinc_device_s16, syldet_recordings_load_sinc_pcm_device: the files at the
    // network's rate are copied), fp32 rows.
    // The upload is the files' data chunks as they are stored.  A batch of 16-bit files is an int16 array (int16 rows, as ever);
    // any other batch is bytes, every file in its own sample format, decoded as the rows load (syldet_recordings_load_pcm_device):
    // no sample is converted on the host.
    std::vector<int64_t> lengths, src_offset, src_samples;
    std::vector<double> src_rate;
    std::vector<int32_t> network, src_step, src_format;
    const size_t el = all16 ? sizeof(int16_t) : 1;          // the unit of the offsets and steps: int16 elements, or bytes
    std::vector<int64_t> file_at(files.size());             // where a file's frames lie in the upload, in that unit (whole 16 bytes)
    int64_t total = 0;
    for (size_t i = 0; i < files.size(); i++) {
        const BatchFile &f = files[i];
        const int64_t sample = all16 ? 1 : f.sample_bytes();
        file_at[i] = total;
        for (int t = 0; t < f.info.channels; t++) {
            lengths.push_back(converting ? syldet_convert_rate_count(f.info.frames, f.info.rate, cfg->sampling_rate) : f.info.frames);
            src_samples.push_back(f.info.frames);
            src_rate.push_back(f.info.rate);
            network.push_back(t);
            src_offset.push_back(total + t * sample);
            src_step.push_back((int32_t)(f.info.channels * sample));
            src_format.push_back(f.format());
        }
        total += ((int64_t)(f.raw.size() / el) + (int64_t)(16 / el) - 1) / (int64_t)(16 / el) * (int64_t)(16 / el);
    }
    const int32_t K = (int32_t)lengths.size();
    // the tracks' destination: file i's frames [n_i][tracks] at frames_at[i], n_i its length at the network's rate
    std::vector<int64_t> dst_offset, frames_at(files.size());
    std::vector<int32_t> dst_step;
    int64_t dst_total = 0;
    for (size_t i = 0, k = 0; i < files.size(); i++) {
        const int tracks = files[i].info.channels;
        frames_at[i] = dst_total;
        for (int t = 0; t < tracks; t++) {
            dst_offset.push_back(dst_total + t);
            dst_step.push_back(tracks);
        }
        dst_total += (lengths[k] * tracks + 7) / 8 * 8;
        k += (size_t)tracks;
    }
    std::vector<int16_t> sim_frames, ttl_frames;            // (zeros where no file of the batch has an evaluation)
    std::vector<int64_t> on_idx, on_cnt;
    int64_t on_cap = 1;
    // --levels-dir: the two tables of every recording, flat as syldet_recordings_levels_layout lays them, and which readings have
    // no evaluation
    const bool metering = !dirs.levels.empty();
    const double lv_per = levels.period * cfg->sampling_rate / (double)levels.buffer;
    const int64_t lv_P = lv_per >= 1.0 ? (lv_per < 9e18 ? (int64_t)lv_per : INT64_MAX) : 1;   // (process_file's)
    std::vector<int64_t> lv_first((size_t)K + 1, 0);
    std::vector<double> lv_in;
    std::vector<float> lv_out;
    std::vector<char> lv_empty;
    // --align-dir: every recording's events, their windows (recording k's from al_begin[k]), and what decides presence
    std::vector<std::vector<int64_t>> al_events;
    std::vector<int64_t> al_units, al_begin;
    std::vector<float> al_windows;
    int64_t al_origin = 0, al_step = 1;
    bool al_made = false;
    try {
        if (!dirs.simulate.empty()) sim_frames.assign((size_t)dst_total, 0);
        if (!dirs.ttl.empty()) ttl_frames.assign((size_t)dst_total, 0);
        if (!dirs.onsets.empty()) on_cnt.assign((size_t)K, 0);
    } catch (const std::bad_alloc &) {
        std::fprintf(stderr, "Unable to process the batch: out of memory.\n");
        files.clear();
        return 2;
    }
    const int n_nets = (int)cfgs.size();
    const int C = (int)std::max<long>(n_nets, std::min<long>(max_rows, K));
    syldet_t *h = nullptr;
    syldet_recordings_t *r = nullptr;
    hipStream_t stream = nullptr;
    std::vector<int32_t> row_net((size_t)C);
    for (int c = 0; c < C; c++) row_net[(size_t)c] = c % n_nets;
    std::vector<int64_t> idx, cnt((size_t)K, 0);
    std::vector<float> val;
    int64_t cap = 1;
    int n_out = 0;
    int rc = 0;
    // --score: the recordings' labels in the recordings' order (a track without labels, or with an evaluation-less file, still
    // counts: its labels are misses at every threshold)
    std::vector<int64_t> score_labels, score_begin(1, 0);
    if (score) {
        for (const BatchFile &f : files) {
            const auto of_file = score->labels.find(f.path);
            for (int t = 0; t < f.info.channels; t++) {
                if (of_file != score->labels.end()) {
                    const auto of_track = of_file->second.find(t);
                    if (of_track != of_file->second.end()) score_labels.insert(score_labels.end(), of_track->second.begin(), of_track->second.end());
                }
                score_begin.push_back((int64_t)score_labels.size());
            }
        }
        score->n_labels += (int64_t)score_labels.size();
    }
    do {
        if (int st = n_nets > 1 ? syldet_create_mixed(cfgs.data(), n_nets, row_net.data(), C, device, SYLDET_ENGINE_AUTO, &h)
                                : syldet_create(cfg, C, device, SYLDET_ENGINE_AUTO, &h)) {
            std::fprintf(stderr, "Unable to create the detector: %s: %s\n", syldet_strerror(st), syldet_last_error());
            rc = 2;
            break;
        }
        syldet_geometry_t g;
        syldet_get_geometry(h, &g);
        n_out = g.outputs;
        int st = syldet_recordings_create(h, lengths.data(), n_nets > 1 ? network.data() : nullptr, K, &r);
        int64_t row_samples = 0, row_evals = 0;
        if (!st) st = syldet_recordings_shape(r, nullptr, &row_samples, &row_evals, nullptr);
        if (st) {
            std::fprintf(stderr, "Unable to plan the batch: %s: %s\n", syldet_strerror(st), syldet_last_error());
            rc = 2;
            break;
        }
        const bool ran = row_evals > 0;
        if (!ran && !metering && !g_align) break;                       // every file shorter than one evaluation: no events (the input meter reads them all the same)
        if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&stream) != hipSuccess) { rc = 2; break; }
        DevBuf d_src, d_rows, d_out, d_flags, d_idx, d_val, d_cnt;
        if (!d_src.alloc((size_t)total * el) || !d_rows.alloc((size_t)C * row_samples * (converting || !all16 ? sizeof(float) : sizeof(int16_t))) || !d_out.alloc((size_t)C * row_evals * n_out * sizeof(float)) ||
            !d_flags.alloc((size_t)C * row_evals) || !d_cnt.alloc((size_t)K * sizeof(int64_t))) { rc = 2; break; }
        bool ok = true;
        for (size_t i = 0; ok && i < files.size(); i++) {
            const BatchFile &f = files[i];
            ok = hipMemcpyAsync((char *)d_src.p + (size_t)file_at[i] * el, f.raw.data(), f.raw.size(), hipMemcpyHostToDevice, stream) == hipSuccess;
        }
        if (!ok) { rc = 2; break; }
        if (converting) {
            st = all16 ? syldet_recordings_load_sinc_device_s16(r, (const int16_t *)d_src.p, src_offset.data(), src_step.data(), src_samples.data(), src_rate.data(),
                                                                conv.zero_crossings, conv.beta, conv.rolloff, (float *)d_rows.p, row_samples, stream)
                       : syldet_recordings_load_sinc_pcm_device(r, d_src.p, total, src_offset.data(), src_step.data(), src_format.data(), src_samples.data(),
                                                                src_rate.data(), conv.zero_crossings, conv.beta, conv.rolloff, (float *)d_rows.p, row_samples, stream);
            if (!st && ran) st = syldet_run_device(h, (const float *)d_rows.p, row_samples, row_samples, (float *)d_out.p, (uint8_t *)d_flags.p, stream);
        } else if (all16) {
            st = syldet_recordings_load_device_s16(r, (const int16_t *)d_src.p, src_offset.data(), src_step.data(), (int16_t *)d_rows.p, row_samples, stream);
            if (!st && ran) st = syldet_run_device_s16(h, (const int16_t *)d_rows.p, row_samples, row_samples, (float *)d_out.p, (uint8_t *)d_flags.p, stream);
        } else {
            st = syldet_recordings_load_pcm_device(r, d_src.p, total, src_offset.data(), src_step.data(), src_format.data(), (float *)d_rows.p, row_samples, stream);
            if (!st && ran) st = syldet_run_device(h, (const float *)d_rows.p, row_samples, row_samples, (float *)d_out.p, (uint8_t *)d_flags.p, stream);
        }
        // --align-dir: the windows of every recording's events, from the batch's arrays on the device (the outputs; the fp32 rows -- a
        // batch of 16-bit files is loaded once more, as fp32, from the same upload --; the rows' columns), in one launch
        DevBuf d_al_rows, d_al_cols;
        auto aligned = [&]() -> bool {
            if (!g_align || st) return true;
            AlignRun &run = *g_align;
            if (syldet_align_anchor(h, run.opt.source, &al_origin, &al_step, nullptr)) {
                std::fprintf(stderr, "Unable to align the events of the batch: %s: %s\n", syldet_strerror(SYLDET_ERR_UNSUPPORTED), syldet_last_error());
                return true;
            }
            al_events.clear();
            int32_t k = 0;
            for (const BatchFile &f : files)
                for (int t = 0; t < f.info.channels; t++, k++) {
                    std::vector<int64_t> found;
                    for (int64_t i = 0; ran && !run.opt.at_labels && i < cnt[(size_t)k]; i++) found.push_back(idx[(size_t)k * (size_t)cap + (size_t)i]);
                    al_events.push_back(align_events_of(run, f.path, t, found));
                }
            std::vector<syldet_slot_t> slots((size_t)std::max<int32_t>(K, 1));
            int ast = syldet_recordings_slots(r, slots.data());
            const float *rows = (const float *)d_rows.p, *src = nullptr;
            int64_t n_units = 0;
            if (!ast && run.opt.source != SYLDET_ALIGN_OUTPUTS && all16 && !converting) {
                std::vector<int64_t> off2(src_offset);
                std::vector<int32_t> step2(src_step);
                for (int64_t &o : off2) o *= 2;
                for (int32_t &q : step2) q *= 2;
                if (!d_al_rows.alloc((size_t)C * (size_t)row_samples * sizeof(float))) return false;
                ast = syldet_recordings_load_pcm_device(r, d_src.p, total * 2, off2.data(), step2.data(), src_format.data(), (float *)d_al_rows.p, row_samples, stream);
                rows = (const float *)d_al_rows.p;
            }
            const int64_t J = std::max<int64_t>(0, syldet_count_frames(h, row_samples));
            al_units.assign((size_t)K, 0);
            if (run.opt.source == SYLDET_ALIGN_SAMPLES) {
                src = rows;
                n_units = row_samples;
                for (int32_t i = 0; i < K; i++) al_units[(size_t)i] = slots[(size_t)i].n_samples;
            } else if (run.opt.source == SYLDET_ALIGN_COLUMNS) {
                if (!d_al_cols.alloc((size_t)C * (size_t)J * (size_t)run.width * sizeof(float))) return false;
                if (!ast && J > 0) ast = syldet_spectrogram_device(h, rows, row_samples, row_samples, (float *)d_al_cols.p, stream);
                src = (const float *)d_al_cols.p;
                n_units = J;
                for (int32_t i = 0; i < K; i++) al_units[(size_t)i] = std::max<int64_t>(0, syldet_count_frames(h, slots[(size_t)i].n_samples));
            } else {
                src = (const float *)d_out.p;
                n_units = row_evals;
                for (int32_t i = 0; i < K; i++) al_units[(size_t)i] = slots[(size_t)i].n_evals;
            }
            if (ast) {
                std::fprintf(stderr, "Unable to align the events of the batch: %s: %s\n", syldet_strerror(ast), syldet_last_error());
                return true;
            }
            al_made = align_windows(run, h, r, src, n_units, 0, al_events, stream, al_windows, al_begin);
            return true;
        };
        // the level tables of every file of the batch: the input meter on the very rows that are run (int16 rows for 16-bit files, fp32
        // rows for float files and for converted ones), the output meter on the outputs the run left; only the two tables come back
        DevBuf d_lv_in, d_lv_out;
        if (!st && metering) {
            int64_t n_readings = 0;
            std::vector<syldet_slot_t> slots((size_t)std::max<int32_t>(K, 1));
            st = syldet_recordings_levels_layout(r, levels.buffer, lv_P, lv_first.data(), &n_readings);
            if (!st) st = syldet_recordings_slots(r, slots.data());
            if (!st) {
                lv_in.assign((size_t)n_readings, 0.0);
                lv_out.assign((size_t)n_readings, 0.0f);
                lv_empty.assign((size_t)n_readings, 1);
                for (int32_t k = 0; k < K; k++)
                    for (int64_t m = 0; m < lv_first[(size_t)k + 1] - lv_first[(size_t)k]; m++) {
                        int64_t first = 0, count = 0;
                        if (syldet_levels_eval_range(h, slots[(size_t)k].n_samples, slots[(size_t)k].n_evals, levels.buffer, lv_P, m, &first, &count) == SYLDET_OK)
                            lv_empty[(size_t)(lv_first[(size_t)k] + m)] = count == 0;
                    }
                if (!d_lv_in.alloc((size_t)n_readings * sizeof(double)) || !d_lv_out.alloc((size_t)n_readings * sizeof(float))) { rc = 2; break; }
            }
            if (!st && n_readings > 0) {
                st = all16 && !converting ? syldet_recordings_levels_device_s16(r, (const int16_t *)d_rows.p, row_samples, levels.buffer, lv_P, (double *)d_lv_in.p, n_readings, stream)
                                          : syldet_recordings_levels_device(r, (const float *)d_rows.p, row_samples, levels.buffer, lv_P, (double *)d_lv_in.p, n_readings, stream);
                if (!st) st = syldet_recordings_output_levels_device(r, ran ? (const float *)d_out.p : nullptr, 0, levels.buffer, lv_P, (float *)d_lv_out.p, n_readings, stream);
                if (!st && (hipMemcpyAsync(lv_in.data(), d_lv_in.p, lv_in.size() * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
                            hipMemcpyAsync(lv_out.data(), d_lv_out.p, lv_out.size() * sizeof(float), hipMemcpyDeviceToHost, stream) != hipSuccess)) { rc = 2; break; }
            }
            if (st) {
                std::fprintf(stderr, "Unable to meter the batch: %s: %s\n", syldet_strerror(st), syldet_last_error());
                rc = 2;
                break;
            }
        }
        if (!st && !ran) {                                  // no file of the batch has an evaluation: no events (labels may still be aligned)
            if (!aligned() || hipStreamSynchronize(stream) != hipSuccess) rc = 2;
            break;
        }
        // the counts first (a scan of the flags), then the detections themselves into tables of the size they need
        if (!st) st = syldet_recordings_events_device(r, nullptr, (const uint8_t *)d_flags.p, debounce_s, nullptr, nullptr, 0, (int64_t *)d_cnt.p, stream);
        if (st) {
            std::fprintf(stderr, "Unable to process the batch: %s: %s\n", syldet_strerror(st), syldet_last_error());
            rc = 2;
            break;
        }
        if (hipMemcpyAsync(cnt.data(), d_cnt.p, cnt.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) { rc = 2; break; }
        cap = std::max<int64_t>(1, *std::max_element(cnt.begin(), cnt.end()));
        idx.resize((size_t)K * (size_t)cap);
        val.resize((size_t)K * (size_t)cap * (size_t)n_out);
        if (!d_idx.alloc(idx.size() * sizeof(int64_t)) || !d_val.alloc(val.size() * sizeof(float))) { rc = 2; break; }
        st = syldet_recordings_events_device(r, (const float *)d_out.p, (const uint8_t *)d_flags.p, debounce_s, (int64_t *)d_idx.p, (float *)d_val.p, cap,
                                             (int64_t *)d_cnt.p, stream);
        if (st) {
            std::fprintf(stderr, "Unable to process the batch: %s: %s\n", syldet_strerror(st), syldet_last_error());
            rc = 2;
            break;
        }
        if (hipMemcpyAsync(idx.data(), d_idx.p, idx.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipMemcpyAsync(val.data(), d_val.p, val.size() * sizeof(float), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) { rc = 2; break; }
        if (score && !score->failed) {
            // the thresholds' tables of every recording in one launch over the outputs that are on the device already
            const int32_t n_thr = (int32_t)score->thresholds.size();
            syldet_scorer_t *sc = nullptr;
            DevBuf d_table;
            std::vector<int64_t> table((size_t)K * (size_t)n_thr * SYLDET_SCORE_COLUMNS);
            st = syldet_scorer_create(h, r, score->thresholds.data(), n_thr, score_labels.data(), score_begin.data(), score->tolerance, debounce_s, &sc);
            if (!st && !d_table.alloc(table.size() * sizeof(int64_t))) { syldet_scorer_destroy(sc); rc = 2; break; }
            if (!st) st = syldet_score_device(sc, (const float *)d_out.p, row_evals, score->output, (int64_t *)d_table.p, stream);
            if (st) {
                std::fprintf(stderr, "Unable to score the batch: %s: %s\n", syldet_strerror(st), syldet_last_error());
                score->failed = true;
            } else if (hipMemcpyAsync(table.data(), d_table.p, table.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
                       hipStreamSynchronize(stream) != hipSuccess) {
                syldet_scorer_destroy(sc);
                rc = 2;
                break;
            } else {
                for (size_t i = 0; i < table.size(); i++) score->totals[i % ((size_t)n_thr * SYLDET_SCORE_COLUMNS)] += table[i];
            }
            syldet_scorer_destroy(sc);
        }
        if (!aligned()) { rc = 2; break; }
        // the tracks of every file of the batch, from the outputs and flags that are on the device
        if (dirs.any()) {
            DevBuf d_sim, d_ttl, d_on_idx, d_on_cnt;
            const int64_t N = ttl.width_samples(cfg->sampling_rate), lat = ttl.latency_samples(cfg->sampling_rate);
            if (!dirs.simulate.empty()) {
                if (!d_sim.alloc((size_t)dst_total * sizeof(int16_t))) { rc = 2; break; }
                st = syldet_recordings_trace_device_s16(r, (const float *)d_out.p, simulate_output, (int16_t *)d_sim.p, dst_total, dst_offset.data(), dst_step.data(), stream);
                if (!st && hipMemcpyAsync(sim_frames.data(), d_sim.p, (size_t)dst_total * sizeof(int16_t), hipMemcpyDeviceToHost, stream) != hipSuccess) { rc = 2; break; }
            }
            if (!st && !dirs.ttl.empty()) {
                if (!d_ttl.alloc((size_t)dst_total * sizeof(int16_t))) { rc = 2; break; }
                st = syldet_recordings_trigger_device_s16(r, (const uint8_t *)d_flags.p, ttl.buffer, N, lat, (int16_t *)d_ttl.p, dst_total, dst_offset.data(), dst_step.data(), stream);
                if (!st && hipMemcpyAsync(ttl_frames.data(), d_ttl.p, (size_t)dst_total * sizeof(int16_t), hipMemcpyDeviceToHost, stream) != hipSuccess) { rc = 2; break; }
            }
            if (!st && !dirs.onsets.empty()) {
                std::vector<syldet_slot_t> slots((size_t)K);
                st = syldet_recordings_slots(r, slots.data());
                for (const syldet_slot_t &sl : slots) on_cap = std::max<int64_t>(on_cap, std::min<int64_t>(sl.n_evals, sl.n_samples / ttl.buffer + 1));
                on_idx.assign((size_t)K * (size_t)on_cap, 0);
                if (!d_on_idx.alloc(on_idx.size() * sizeof(int64_t)) || !d_on_cnt.alloc(on_cnt.size() * sizeof(int64_t))) { rc = 2; break; }
                if (!st) st = syldet_recordings_trigger_onsets_device(r, (const uint8_t *)d_flags.p, ttl.buffer, N, lat, (int64_t *)d_on_idx.p, on_cap, (int64_t *)d_on_cnt.p, stream);
                if (!st && (hipMemcpyAsync(on_idx.data(), d_on_idx.p, on_idx.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
                            hipMemcpyAsync(on_cnt.data(), d_on_cnt.p, on_cnt.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream) != hipSuccess)) { rc = 2; break; }
            }
            if (st) {
                std::fprintf(stderr, "Unable to make the tracks of the batch: %s: %s\n", syldet_strerror(st), syldet_last_error());
                rc = 2;
                break;
            }
            if (hipStreamSynchronize(stream) != hipSuccess) { rc = 2; break; }
        }
    } while (false);
    if (rc == 2 && hipPeekAtLastError() != hipSuccess) std::fprintf(stderr, "Unable to process the batch: %s\n", hipGetErrorString(hipGetLastError()));
    if (stream) (void)hipStreamDestroy(stream);
    syldet_recordings_destroy(r);
    syldet_destroy(h);
    if (rc && score) score->failed = true;                  // (a table without this batch would be another archive's)
    // file by file, the lines process_file prints: the tracks' events interleaved buffer by buffer (main.swift:126-130)
    int32_t k0 = 0;
    bool unwritten = false;
    for (const BatchFile &f : files) {
        if (headers) std::printf("%s\n", f.path.c_str());  // main.swift:122-124
        std::vector<Event> events;
        for (int c = 0; !rc && c < f.info.channels; c++)
            for (int64_t i = 0; i < cnt[(size_t)(k0 + c)]; i++) {
                const int64_t smp = idx[(size_t)(k0 + c) * (size_t)cap + (size_t)i];
                events.push_back({chunk > 0 ? (smp - 1) / chunk : 0, c, smp, i});
            }
        std::stable_sort(events.begin(), events.end(), [](const Event &a, const Event &b) {
            if (a.buffer != b.buffer) return a.buffer < b.buffer;
            if (a.channel != b.channel) return a.channel < b.channel;
            return a.sample < b.sample;
        });
        for (const Event &ev : events) {
            std::string line = std::to_string(ev.channel) + "," + std::to_string(ev.sample) + "," + number((double)ev.sample / cfg->sampling_rate);
            for (int o = 0; o < n_out; o++) line += "," + number(val[((size_t)(k0 + ev.channel) * (size_t)cap + (size_t)ev.eval) * n_out + o]);
            std::puts(line.c_str());
        }
        std::fflush(stdout);
        // the file's tracks behind its lines, which a failing write must not cost (process_file's order and its messages)
        if (!rc && dirs.any()) {
            const size_t i = (size_t)(&f - files.data());
            const int tracks = f.info.channels;
            const int64_t n = lengths[(size_t)k0];
            std::string werr;
            const std::string sim = TrackDirs::in(dirs.simulate, f.path), trg = TrackDirs::in(dirs.ttl, f.path), ons = TrackDirs::in(dirs.onsets, f.path, ".tsv");
            if (!sim.empty() && !wav::write_s16(sim, cfg->sampling_rate, tracks, n, sim_frames.data() + frames_at[i], werr)) {
                std::fprintf(stderr, "Unable to write %s: %s\n", sim.c_str(), werr.c_str());
                unwritten = true;
            }
            if (!trg.empty() && !wav::write_s16(trg, cfg->sampling_rate, tracks, n, ttl_frames.data() + frames_at[i], werr)) {
                std::fprintf(stderr, "Unable to write %s: %s\n", trg.c_str(), werr.c_str());
                unwritten = true;
            }
            if (!ons.empty() && !write_onsets(ons, tracks, on_idx.empty() ? nullptr : on_idx.data() + (size_t)k0 * (size_t)on_cap, on_cnt.data() + k0, on_cap, cfg->sampling_rate)) {
                std::fprintf(stderr, "Unable to write %s.\n", ons.c_str());
                unwritten = true;
            }
        }
        // ... its windows at the events, with their table (process_file's files)
        if (!rc && g_align) {
            const int tracks = f.info.channels;
            if (!al_made) unwritten = true;
            else if (align_write_file(*g_align, f.path, std::vector<std::vector<int64_t>>(al_events.begin() + k0, al_events.begin() + k0 + tracks),
                                      std::vector<int64_t>(al_units.begin() + k0, al_units.begin() + k0 + tracks),
                                      al_windows.data() + (size_t)al_begin[(size_t)k0] * (size_t)g_align->L(), al_origin, al_step, cfg->sampling_rate))
                unwritten = true;
        }
        // ... and its level table, line for line what process_file writes: reading by reading, track by track
        if (!rc && metering) {
            const std::string tsv = TrackDirs::in(dirs.levels, f.path, ".tsv");
            const int tracks = f.info.channels;
            const int64_t fed = lengths[(size_t)k0], M = lv_first[(size_t)k0 + 1] - lv_first[(size_t)k0];
            const int64_t PL = std::min(lv_P, (fed + levels.buffer - 1) / levels.buffer) * levels.buffer;
            FILE *out = std::fopen(tsv.c_str(), "w");
            bool ok = out != nullptr;
            for (int64_t m = 0; ok && m < M; m++)
                for (int c = 0; ok && c < tracks; c++) {
                    const size_t at = (size_t)(lv_first[(size_t)(k0 + c)] + m);
                    const std::string line = std::to_string(c) + "\t" + number((double)std::min((m + 1) * PL, fed) / cfg->sampling_rate) + "\t" +
                                             number(std::sqrt(lv_in[at])) + "\t" + (lv_empty[at] ? std::string() : number(lv_out[at])) + "\n";
                    ok = std::fputs(line.c_str(), out) >= 0;
                }
            if (out && std::fclose(out) != 0) ok = false;
            if (!ok) {
                std::fprintf(stderr, "Unable to write %s.\n", tsv.c_str());
                unwritten = true;
            }
        }
        k0 += f.info.channels;
    }
    files.clear();
    return rc ? rc : (unwritten ? 3 : 0);
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

// The loop over the -a files under --batch: consecutive files that can share a bank (readable, the right number of tracks, at the
// network's rate or -- under --resample sinc -- at a rate the band-limited converter takes) gather until their samples pass
// opt.bytes; any other file ends the batch and is processed alone in its place.
int process_batched(const std::vector<std::string> &audio, const std::vector<syldet_config_t *> &cfgs, int device, double debounce_s, bool have_debounce,
                    int64_t chunk, const BatchOpt &opt, const ResampleOpt &conv, ScoreRun *score, const TrackDirs &dirs, int simulate_output, const TtlOpt &ttl,
                    const LevelsOpt &levels)
{
    int rc = 0;
    const bool headers = audio.size() > 1;
    const double deb = have_debounce ? debounce_s : 0.0;
    std::vector<BatchFile> files;
    size_t held = 0;
    // what --align-dir adds to a batch on the device, per sample at the file's rate: the columns (4 x bins / hop bytes), the fp32 rows
    // the samples are cut from (4 bytes), nothing for the outputs
    double align_bytes_per_sample = 0.0;
    if (g_align) {
        syldet_geometry_t g;
        if (syldet_config_geometry(cfgs[0], &g) == SYLDET_OK)
            align_bytes_per_sample = g_align->opt.source == SYLDET_ALIGN_COLUMNS ? 4.0 + 4.0 * g.bins / g.hop : g_align->opt.source == SYLDET_ALIGN_SAMPLES ? 4.0 : 0.0;
    }
    auto flush = [&]() {
        const int r = run_batch(files, cfgs, device, deb, chunk, opt.rows, headers, score, conv, dirs, simulate_output, ttl, levels);
        if (r == 2) rc = 2;
        else if (r == 3 && rc == 0) rc = 1;
        held = 0;
    };
    for (const std::string &p : audio) {
        BatchFile f;
        f.path = p;
        std::string err;
        const bool probed = wav::probe(p, f.info, err);
        // (syldet_sinc_taps is -1 for what the converter refuses: a ratio outside [1/16, 16], a filter too wide)
        f.convert = probed && f.info.rate != cfgs[0]->sampling_rate;
        const bool rate_ok = probed && (!f.convert || (conv.sinc && syldet_sinc_taps(f.info.rate, cfgs[0]->sampling_rate, conv.zero_crossings, conv.rolloff) >= 0));
        if (probed && rate_ok && f.info.channels > 0 && f.info.frames > 0 &&
            (cfgs.size() == 1 || (size_t)f.info.channels == cfgs.size())) {
            f.is16 = f.info.format == 1 && f.info.bits == 16;
            err.clear();
            if (wav::read_raw(p, f.info, f.raw, err)) {
                held += f.bytes() + (size_t)((double)f.info.frames * (double)f.info.channels * align_bytes_per_sample);
                files.push_back(std::move(f));
                if ((long long)held >= opt.bytes) flush();
                continue;
            }
        }
        // another rate that does not join the bank, unreadable, no tracks, the wrong number of tracks: exactly as without --batch, in its place
        flush();
        if (score && score->labels.count(p)) std::fprintf(stderr, "--score: %s does not go through the bank; its labels are left out.\n", p.c_str());
        if (headers) std::printf("%s\n", p.c_str());
        std::fflush(stdout);
        const int r = process_file(p, cfgs, device, debounce_s, have_debounce, chunk, dirs.simulate_for(p, std::string()), simulate_output,
                                   dirs.levels.empty() ? LevelsOpt() : dirs.levels_for(p, levels), dirs.any() ? dirs.ttl_for(p, ttl) : TtlOpt(), conv);
        if (r == 2) rc = 2;
        else if (r == 3 && rc == 0) rc = 1;
    }
    flush();
    return rc;
}

}  // namespace

int main(int argc, char **argv)
{
    std::vector<std::string> net;
    std::vector<std::string> audio;
    std::string simulate;
    bool have_simulate = false, have_simulate_output = false;
    int simulate_output = 0;
    double debounce = 0.0;
    bool have_debounce = false, probe = false;
    ResampleOpt conv;
    bool have_resample_quality = false;
    syldet_sinc_defaults(&conv.zero_crossings, &conv.beta, &conv.rolloff);
    LevelsOpt levels;
    bool have_levels = false, have_levels_option = false;
    TtlOpt ttl;
    bool have_ttl = false, have_ttl_onsets = false, have_ttl_option = false, have_ttl_width = false, have_ttl_steps = false;
    int device = 0;
    int64_t chunk = 8192;
    BatchOpt batch;
    bool have_batch_option = false;
    TrackDirs dirs;
    bool have_simulate_dir = false, have_ttl_dir = false, have_onsets_dir = false, have_levels_dir = false;
    ScoreOpt score;
    bool have_score = false, have_score_option = false;
    AlignOpt align;
    bool have_align_dir = false, have_align_option = false;
    auto value = [&](int &i, const char *name) -> const char * {
        if (i + 1 >= argc) {
            std::fprintf(stderr, "Missing value for %s.\n", name);
            usage(stdout);
            std::exit(kExUsage);
        }
        return argv[++i];
    };
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "-n" || a == "--net") net.push_back(value(i, "--net"));
        else if (a == "-a" || a == "--audio") audio.push_back(value(i, "--audio"));
        else if (a == "-d" || a == "--debounce") {
            const char *v = value(i, "--debounce");
            char *end = nullptr;
            debounce = std::strtod(v, &end);
            have_debounce = end && *end == 0 && end != v;   // Double.init(String): nil (no debounce) when not a number
        } else if (a == "--device") device = std::atoi(value(i, "--device"));
        else if (a == "--chunk") chunk = std::atoll(value(i, "--chunk"));
        else if (a == "--probe") probe = true;
        else if (a == "--batch") batch.on = true;
        else if (a == "--batch-rows" || a == "--batch-bytes") {
            const bool rows = a == "--batch-rows";
            const char *v = value(i, a.c_str());
            char *end = nullptr;
            const long long k = std::strtoll(v, &end, 10);
            if (end == v || *end != 0 || k < 1 || (rows && k > 65535)) {
                std::fprintf(stderr, rows ? "--batch-rows takes a number of rows from 1 to 65535.\n" : "--batch-bytes takes a number of bytes, 1 or more.\n");
                usage(stdout);
                return kExUsage;
            }
            if (rows) batch.rows = (long)k;
            else batch.bytes = k;
            have_batch_option = true;
        }
        else if (a == "--score") { score.labels_path = value(i, "--score"); have_score = true; }
        else if (a == "--score-out") { score.out_path = value(i, "--score-out"); have_score_option = true; }
        else if (a == "--score-thresholds") {
            // lo:hi:n, the grid lo + (hi - lo) i / (n - 1)
            const std::string v = value(i, "--score-thresholds");
            const size_t c1 = v.find(':'), c2 = c1 == std::string::npos ? c1 : v.find(':', c1 + 1);
            char *e1 = nullptr, *e2 = nullptr, *e3 = nullptr;
            const std::string lo = v.substr(0, c1), hi = c2 == std::string::npos ? "" : v.substr(c1 + 1, c2 - c1 - 1), n = c2 == std::string::npos ? "" : v.substr(c2 + 1);
            score.lo = std::strtod(lo.c_str(), &e1);
            score.hi = std::strtod(hi.c_str(), &e2);
            score.n = std::strtol(n.c_str(), &e3, 10);
            if (lo.empty() || hi.empty() || n.empty() || *e1 || *e2 || *e3 || std::isnan(score.lo) || std::isnan(score.hi) || score.n < 1 ||
                score.n > SYLDET_SCORE_MAX_THRESHOLDS) {
                std::fprintf(stderr, "--score-thresholds takes lo:hi:n, two numbers and a count from 1 to %d.\n", SYLDET_SCORE_MAX_THRESHOLDS);
                usage(stdout);
                return kExUsage;
            }
            have_score_option = true;
        }
        else if (a == "--score-tolerance" || a == "--score-cost") {
            const bool tol = a == "--score-tolerance";
            const char *v = value(i, a.c_str());
            char *end = nullptr;
            const double x = std::strtod(v, &end);
            if (end == v || *end != 0 || !(x >= 0.0) || std::isinf(x)) {
                std::fprintf(stderr, "%s takes a number, 0 or more.\n", a.c_str());
                usage(stdout);
                return kExUsage;
            }
            (tol ? score.tolerance : score.cost) = x;
            have_score_option = true;
        }
        else if (a == "--score-output") {
            const char *v = value(i, "--score-output");
            char *end = nullptr;
            const long k = std::strtol(v, &end, 10);
            if (end == v || *end != 0 || k < 0 || k > 65535) {
                std::fprintf(stderr, "--score-output takes the number of a network output, 0 or more.\n");
                usage(stdout);
                return kExUsage;
            }
            score.output = (int)k;
            have_score_option = true;
        }
        else if (a == "--align-dir") {
            align.dir = value(i, "--align-dir");
            have_align_dir = true;
        } else if (a == "--align" || a == "--align-at") {
            const bool src = a == "--align";
            const std::string v = value(i, a.c_str());
            if (src ? (v != "columns" && v != "outputs" && v != "samples") : (v != "detections" && v != "labels")) {
                std::fprintf(stderr, src ? "--align takes columns, outputs or samples.\n" : "--align-at takes detections or labels.\n");
                usage(stdout);
                return kExUsage;
            }
            if (src) align.source = v == "columns" ? SYLDET_ALIGN_COLUMNS : v == "outputs" ? SYLDET_ALIGN_OUTPUTS : SYLDET_ALIGN_SAMPLES;
            else align.at_labels = v == "labels";
            have_align_option = true;
        } else if (a == "--align-before" || a == "--align-after") {
            const bool b = a == "--align-before";
            const char *v = value(i, a.c_str());
            char *end = nullptr;
            const long k = std::strtol(v, &end, 10);
            if (end == v || *end != 0 || k < 0 || k > SYLDET_ALIGN_MAX_WINDOW) {
                std::fprintf(stderr, "--align-before and --align-after take a number of units, 0 or more.\n");
                usage(stdout);
                return kExUsage;
            }
            (b ? align.before : align.after) = k;
            have_align_option = true;
        }
        else if (a == "--resample") {
            const std::string m = value(i, "--resample");
            if (m != "linear" && m != "sinc") {
                std::fprintf(stderr, "--resample takes linear or sinc.\n");
                usage(stdout);
                return kExUsage;
            }
            conv.sinc = m == "sinc";
        } else if (a == "--resample-quality") {
            // Z,beta,rolloff: three numbers, nothing else, inside the converter's ranges (syldet_sinc_taps knows Z's and rolloff's)
            const char *v = value(i, "--resample-quality");
            char *e1 = nullptr, *e2 = nullptr, *e3 = nullptr;
            const long z = std::strtol(v, &e1, 10);
            const double b = e1 != v && *e1 == ',' ? std::strtod(e1 + 1, &e2) : 0.0;
            const double r = e2 && e2 != e1 + 1 && *e2 == ',' ? std::strtod(e2 + 1, &e3) : 0.0;
            if (!e3 || e3 == e2 + 1 || *e3 != 0 || z < 4 || z > 64 || !(b >= 0.0 && b <= 20.0) || !(r > 0.0 && r <= 1.0)) {
                std::fprintf(stderr, "--resample-quality takes Z,beta,rolloff: 4 to 64 zero crossings, beta from 0 to 20, a rolloff above 0 and at most 1.\n");
                usage(stdout);
                return kExUsage;
            }
            conv.zero_crossings = (int32_t)z; conv.beta = b; conv.rolloff = r;
            have_resample_quality = true;
        }
        else if (a == "--simulate") {
            simulate = value(i, "--simulate");
            have_simulate = true;
        } else if (a == "--simulate-dir") {
            dirs.simulate = value(i, "--simulate-dir");
            have_simulate_dir = true;
        } else if (a == "--levels-dir") {
            dirs.levels = value(i, "--levels-dir");
            have_levels_dir = true;
        } else if (a == "--ttl-dir") {
            dirs.ttl = value(i, "--ttl-dir");
            have_ttl_dir = true;
        } else if (a == "--ttl-onsets-dir") {
            dirs.onsets = value(i, "--ttl-onsets-dir");
            have_onsets_dir = true;
        } else if (a == "--simulate-output") {
            const char *v = value(i, "--simulate-output");
            char *end = nullptr;
            const long k = std::strtol(v, &end, 10);
            if (end == v || *end != 0 || k < 0 || k > 0x7fffffffL) {
                std::fprintf(stderr, "--simulate-output takes an output number (0, 1, ...).\n");
                usage(stdout);
                return kExUsage;
            }
            simulate_output = (int)k;
            have_simulate_output = true;
        }
        else if (a == "--levels") {
            levels.path = value(i, "--levels");
            have_levels = true;
        } else if (a == "--levels-buffer") {
            const char *v = value(i, "--levels-buffer");
            char *end = nullptr;
            const long k = std::strtol(v, &end, 10);
            if (end == v || *end != 0 || k < 8 || k > 4096 || (k & (k - 1)) != 0) {
                std::fprintf(stderr, "--levels-buffer takes a power of two from 8 to 4096.\n");
                usage(stdout);
                return kExUsage;
            }
            levels.buffer = (int)k;
            have_levels_option = true;
        } else if (a == "--levels-period") {
            const char *v = value(i, "--levels-period");
            char *end = nullptr;
            levels.period = std::strtod(v, &end);
            if (end == v || *end != 0 || !(levels.period > 0.0) || levels.period > 1e15) {
                std::fprintf(stderr, "--levels-period takes a positive number of seconds.\n");
                usage(stdout);
                return kExUsage;
            }
            have_levels_option = true;
        }
        else if (a == "--ttl") {
            ttl.path = value(i, "--ttl");
            have_ttl = true;
        } else if (a == "--ttl-onsets") {
            ttl.onsets = value(i, "--ttl-onsets");
            have_ttl_onsets = true;
        } else if (a == "--ttl-mux") {
            ttl.mux = true;
        } else if (a == "--ttl-width" || a == "--ttl-latency") {
            const bool w = a == "--ttl-width";
            const char *v = value(i, a.c_str());
            char *end = nullptr;
            const double x = std::strtod(v, &end);
            if (end == v || *end != 0 || !(w ? x > 0.0 : x >= 0.0) || x > 1e15) {
                std::fprintf(stderr, w ? "--ttl-width takes a positive number of seconds.\n" : "--ttl-latency takes a number of seconds, 0 or more.\n");
                usage(stdout);
                return kExUsage;
            }
            (w ? ttl.width : ttl.latency) = x;
            have_ttl_option = true;
            if (w) have_ttl_width = true;
        } else if (a == "--ttl-steps") {
            const char *v = value(i, "--ttl-steps");
            char *end = nullptr;
            const long k = std::strtol(v, &end, 10);
            if (end == v || *end != 0 || k < 1 || k > (1L << 24)) {
                std::fprintf(stderr, "--ttl-steps takes a number of buffers, 1 or more.\n");
                usage(stdout);
                return kExUsage;
            }
            ttl.steps = k;
            have_ttl_option = have_ttl_steps = true;
        } else if (a == "--ttl-buffer") {
            const char *v = value(i, "--ttl-buffer");
            char *end = nullptr;
            const long k = std::strtol(v, &end, 10);
            if (end == v || *end != 0 || k < 8 || k > 4096 || (k & (k - 1)) != 0) {
                std::fprintf(stderr, "--ttl-buffer takes a power of two from 8 to 4096.\n");
                usage(stdout);
                return kExUsage;
            }
            ttl.buffer = (int)k;
            have_ttl_option = true;
        }
        else if (a == "--format") {
            const std::string f = value(i, "--format");
            if (f != "shortest" && f != "swift4") { usage(stdout); return kExUsage; }
            g_swift4 = f == "swift4";
        } else if (a == "--format-line") {
            // formats one event line from its parts (channel sample rate out0 [out1 ...]; the outputs as fp32) exactly as the
            // event loop does: the known-answer test of the number formats, no audio and no GPU involved
            if (i + 3 >= argc) { usage(stdout); return kExUsage; }
            const long long smp = std::atoll(argv[i + 2]);
            std::string line = std::string(argv[i + 1]) + "," + std::to_string(smp) + "," + number((double)smp / std::strtod(argv[i + 3], nullptr));
            for (int k = i + 4; k < argc; k++) line += "," + number(std::strtof(argv[k], nullptr));
            std::puts(line.c_str());
            return 0;
        } else {                                              // -h, --help and anything unknown: usage text, EX_USAGE (main.swift:27-41)
            usage(stdout);
            return kExUsage;
        }
    }
    if (probe) {
        int bad = 0;
        for (const std::string &p : audio) {
            wav::Info info;
            std::string err;
            if (!wav::probe(p, info, err)) { std::fprintf(stderr, "Unable to read %s: %s\n", p.c_str(), err.c_str()); bad = 1; continue; }
            std::printf("%s: %d channel(s), %s Hz, %s %d-bit, %lld frames\n", p.c_str(), info.channels, swift_number(info.rate).c_str(),
                        info.format == 3 ? "float" : "pcm", info.bits, (long long)info.frames);
        }
        return bad;
    }
    if (net.empty()) {                                      // the option is .required() in the reference (main.swift:21)
        usage(stdout);
        return kExUsage;
    }
    if (have_resample_quality && !conv.sinc) {
        std::fprintf(stderr, "--resample-quality needs --resample sinc.\n");
        usage(stdout);
        return kExUsage;
    }
    if (have_simulate && (audio.size() != 1 || simulate.empty())) {   // the Simulator takes one recording (simulateNetwork(_:withAudio:writeTo:), ViewControllerSimulator.swift:135)
        std::fprintf(stderr, "--simulate writes the track of exactly one audio file (-a).\n");
        usage(stdout);
        return kExUsage;
    }
    if ((have_simulate_dir && dirs.simulate.empty()) || (have_ttl_dir && dirs.ttl.empty()) || (have_onsets_dir && dirs.onsets.empty())) {
        std::fprintf(stderr, "--simulate-dir, --ttl-dir and --ttl-onsets-dir take the name of a directory.\n");
        usage(stdout);
        return kExUsage;
    }
    if ((have_simulate && have_simulate_dir) || (have_ttl && have_ttl_dir) || (have_ttl_onsets && have_onsets_dir)) {
        std::fprintf(stderr, "--simulate-dir, --ttl-dir and --ttl-onsets-dir write what --simulate, --ttl and --ttl-onsets write, for every audio file: give the one or the other.\n");
        usage(stdout);
        return kExUsage;
    }
    if (have_levels_dir && dirs.levels.empty()) {
        std::fprintf(stderr, "--levels-dir takes the name of a directory.\n");
        usage(stdout);
        return kExUsage;
    }
    if (have_levels && have_levels_dir) {
        std::fprintf(stderr, "--levels-dir writes what --levels writes, for every audio file: give the one or the other.\n");
        usage(stdout);
        return kExUsage;
    }
    if (have_align_dir && align.dir.empty()) {
        std::fprintf(stderr, "--align-dir takes the name of a directory.\n");
        usage(stdout);
        return kExUsage;
    }
    if (have_align_option && !have_align_dir) {
        std::fprintf(stderr, "--align, --align-at, --align-before and --align-after need --align-dir <dir>.\n");
        usage(stdout);
        return kExUsage;
    }
    if (align.at_labels && !have_score) {
        std::fprintf(stderr, "--align-at labels needs --score <labels.tsv>.\n");
        usage(stdout);
        return kExUsage;
    }
    if (have_align_dir) {                                   // every audio file's windows go under its own name, beside the three stack files
        std::set<std::string> names = {"count", "sum", "sumsq"};
        for (const std::string &p : audio)
            if (!names.insert(TrackDirs::name_of(p)).second) {
                std::fprintf(stderr, "--align-dir names its files after the audio files (and count, sum, sumsq): two of those are called %s.\n", TrackDirs::name_of(p).c_str());
                usage(stdout);
                return kExUsage;
            }
    }
    if (dirs.any() || have_levels_dir) {                    // every audio file's products go under its own name
        std::set<std::string> names;
        for (const std::string &p : audio)
            if (!names.insert(TrackDirs::name_of(p)).second) {
                std::fprintf(stderr, "--simulate-dir, --ttl-dir, --ttl-onsets-dir and --levels-dir name their files after the audio files: two of those are called %s.\n",
                             TrackDirs::name_of(p).c_str());
                usage(stdout);
                return kExUsage;
            }
    }
    if (ttl.mux && batch.on) {
        std::fprintf(stderr, "--ttl-mux is not available under --batch.\n");
        usage(stdout);
        return kExUsage;
    }
    if (have_simulate_output && !have_simulate && !have_simulate_dir) {
        std::fprintf(stderr, "--simulate-output needs --simulate <out.wav> or --simulate-dir <dir>.\n");
        usage(stdout);
        return kExUsage;
    }
    if (have_levels && (audio.size() != 1 || levels.path.empty())) {   // one table, one recording
        std::fprintf(stderr, "--levels writes the readings of exactly one audio file (-a).\n");
        usage(stdout);
        return kExUsage;
    }
    if (have_levels_option && !have_levels && !have_levels_dir) {
        std::fprintf(stderr, "--levels-buffer and --levels-period need --levels <out.tsv> or --levels-dir <dir>.\n");
        usage(stdout);
        return kExUsage;
    }
    if ((have_ttl && (audio.size() != 1 || ttl.path.empty())) || (have_ttl_onsets && (audio.size() != 1 || ttl.onsets.empty()))) {   // one rig, one recording
        std::fprintf(stderr, "--ttl and --ttl-onsets write the triggers of exactly one audio file (-a).\n");
        usage(stdout);
        return kExUsage;
    }
    if (ttl.mux && !have_ttl && !have_ttl_dir) {
        std::fprintf(stderr, "--ttl-mux needs --ttl <out.wav> or --ttl-dir <dir>.\n");
        usage(stdout);
        return kExUsage;
    }
    if (have_ttl_option && !have_ttl && !have_ttl_onsets && !have_ttl_dir && !have_onsets_dir) {
        std::fprintf(stderr, "--ttl-width, --ttl-steps, --ttl-buffer and --ttl-latency need --ttl <out.wav>, --ttl-onsets <out.tsv>, --ttl-dir <dir> or --ttl-onsets-dir <dir>.\n");
        usage(stdout);
        return kExUsage;
    }
    if (have_ttl_width && have_ttl_steps) {
        std::fprintf(stderr, "--ttl-width and --ttl-steps both set the pulse's width: give one.\n");
        usage(stdout);
        return kExUsage;
    }
    if (have_batch_option && !batch.on) {
        std::fprintf(stderr, "--batch-rows and --batch-bytes need --batch.\n");
        usage(stdout);
        return kExUsage;
    }
    if (batch.on && have_levels) {                          // (one table, one file; a batch's tables go to --levels-dir)
        std::fprintf(stderr, "--levels is not available under --batch: it takes exactly one file and a bank of its own.\n");
        usage(stdout);
        return kExUsage;
    }
    if (batch.on && (have_simulate || have_ttl || have_ttl_onsets)) {   // those name one file; under --batch every file's tracks go to a directory
        std::fprintf(stderr, "--batch runs many files through one bank; --simulate, --ttl and --ttl-onsets take exactly one file: give --simulate-dir, --ttl-dir and --ttl-onsets-dir instead.\n");
        usage(stdout);
        return kExUsage;
    }
    const bool labels_only = have_score && !batch.on && align.at_labels && !have_score_option;   // --score as the file of --align-at labels
    if (have_score && !batch.on && !labels_only) {          // the scorer's detectors are the recordings of a batch
        std::fprintf(stderr, "--score needs --batch.\n");
        usage(stdout);
        return kExUsage;
    }
    if (have_score_option && !have_score) {
        std::fprintf(stderr, "--score-out, --score-thresholds, --score-tolerance, --score-cost and --score-output need --score <labels.tsv>.\n");
        usage(stdout);
        return kExUsage;
    }
    if (have_score && !labels_only && (score.labels_path.empty() || score.out_path.empty())) {
        std::fprintf(stderr, "--score <labels.tsv> needs --score-out <table.tsv>.\n");
        usage(stdout);
        return kExUsage;
    }
    ScoreRun scoring;
    if (have_score) {
        std::string err;
        if (!read_labels(score.labels_path, scoring, err)) {
            std::fprintf(stderr, "--score: %s.\n", err.c_str());
            usage(stdout);
            return kExUsage;
        }
    }
    std::vector<syldet_config_t *> cfgs;
    for (const std::string &n : net) {
        syldet_config_t *cfg = nullptr;
        if (int st = syldet_config_load_text(n.c_str(), &cfg)) {
            std::fprintf(stderr, "Unable to load the network configuration: %s: %s\n", syldet_strerror(st), syldet_last_error());
            for (syldet_config_t *c : cfgs) syldet_config_free(c);
            return 1;
        }
        cfg->rule = SYLDET_RULE_ANY;                        // any output above its threshold, TrackDetector.swift:72-77
        cfgs.push_back(cfg);
    }
    if (have_simulate || have_simulate_dir)                 // (before the GPU is opened)
        for (syldet_config_t *c : cfgs)
            if (simulate_output >= c->n_thresholds) {
                std::fprintf(stderr, "--simulate-output %d: the network has %d output(s).\n", simulate_output, c->n_thresholds);
                for (syldet_config_t *k : cfgs) syldet_config_free(k);
                usage(stdout);
                return kExUsage;
            }
    if (ttl.any() || have_ttl_dir || have_onsets_dir) {     // (before the GPU is opened)
        const double rate = cfgs[0]->sampling_rate;
        const int64_t N = ttl.width_samples(rate), lat = ttl.latency_samples(rate);
        if (N < 1 || N > (1ll << 24) || lat > (1ll << 24)) {
            if (N < 1) std::fprintf(stderr, "--ttl-width: shorter than one sample at %s Hz.\n", swift_number(rate).c_str());
            else std::fprintf(stderr, "The pulse's width and --ttl-latency may be 16777216 samples at most.\n");
            for (syldet_config_t *k : cfgs) syldet_config_free(k);
            usage(stdout);
            return kExUsage;
        }
    }
    if (have_score) {                                       // (before the GPU is opened)
        const double tol = score.tolerance * cfgs[0]->sampling_rate;
        bool ok = tol <= (double)SYLDET_SCORE_MAX_TOLERANCE;
        if (!ok) std::fprintf(stderr, "--score-tolerance may be %d samples at most.\n", SYLDET_SCORE_MAX_TOLERANCE);
        for (syldet_config_t *c : cfgs)
            if (ok && score.output >= c->n_thresholds) {
                std::fprintf(stderr, "--score-output %d: the network has %d output(s).\n", score.output, c->n_thresholds);
                ok = false;
            }
        if (!ok) {
            for (syldet_config_t *k : cfgs) syldet_config_free(k);
            usage(stdout);
            return kExUsage;
        }
        scoring.tolerance = (int64_t)tol;
        scoring.output = score.output;
        for (long i = 0; i < score.n; i++) scoring.thresholds.push_back(score.n > 1 ? score.lo + (score.hi - score.lo) * (double)i / (double)(score.n - 1) : score.lo);
        scoring.totals.assign((size_t)score.n * SYLDET_SCORE_COLUMNS, 0);
    }
    AlignRun aligning;
    if (have_align_dir) {                                   // (before the GPU is opened)
        syldet_geometry_t g;
        const int gst = syldet_config_geometry(cfgs[0], &g);
        aligning.opt = align;
        aligning.labels = &scoring.labels;
        aligning.before = align.before < 0 ? cfgs[0]->time_range - 1 : align.before;
        aligning.after = align.after < 0 ? cfgs[0]->time_range - 1 : align.after;
        aligning.n = aligning.before + aligning.after + 1;
        aligning.width = align.source == SYLDET_ALIGN_COLUMNS ? g.bins : align.source == SYLDET_ALIGN_OUTPUTS ? cfgs[0]->n_thresholds : 1;
        aligning.networks = (int)cfgs.size();
        if (gst || aligning.width < 1 || aligning.L() > SYLDET_ALIGN_MAX_WINDOW) {
            if (gst) std::fprintf(stderr, "Unable to use the network configuration: %s: %s\n", syldet_strerror(gst), syldet_last_error());
            else std::fprintf(stderr, "--align-before and --align-after: a window may hold %d values at most.\n", SYLDET_ALIGN_MAX_WINDOW);
            for (syldet_config_t *k : cfgs) syldet_config_free(k);
            usage(stdout);
            return kExUsage;
        }
        aligning.stacks.resize(cfgs.size());
        for (AlignRun::Stack &st : aligning.stacks) {
            st.count.assign((size_t)aligning.L(), 0);
            st.sum.assign((size_t)aligning.L(), 0.0);
            st.sumsq.assign((size_t)aligning.L(), 0.0);
        }
        std::error_code ec;
        std::filesystem::create_directories(align.dir, ec);
        g_align = &aligning;
    }
    if (batch.on) {
        dirs.make();
        int brc = process_batched(audio, cfgs, device, debounce, have_debounce, chunk, batch, conv, have_score ? &scoring : nullptr, dirs, simulate_output, ttl,
                                  levels);
        for (syldet_config_t *c : cfgs) syldet_config_free(c);
        // the table last, and only a whole one; standard output and the status are those of the run without --score
        if (have_score && (scoring.failed || !write_score_table(score, scoring)) && brc == 0) brc = 1;
        if (g_align && !align_finish(aligning) && brc == 0) brc = 1;
        return brc;
    }
    int rc = 0;
    dirs.make();
    for (const std::string &p : audio) {
        if (audio.size() > 1) std::printf("%s\n", p.c_str());   // main.swift:122-124
        std::fflush(stdout);
        const int r = process_file(p, cfgs, device, debounce, have_debounce, chunk, dirs.simulate_for(p, simulate), simulate_output, dirs.levels_for(p, levels),
                                   dirs.ttl_for(p, ttl), conv);
        if (r == 2) rc = 2;                                 // device trouble is fatal for the exit code; an unreadable file is skipped
        else if (r == 3 && rc == 0) rc = 1;                 // ... and so is a track that could not be written
    }
    for (syldet_config_t *c : cfgs) syldet_config_free(c);
    if (g_align && !align_finish(aligning) && rc == 0) rc = 1;
    return rc;
}
