// The tool's options: what each feature takes, the one struct that holds them all and which were given, the loop that reads them,
// the checks of one option against another, and the usage text.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <set>
#include <string>
#include <vector>

#include "syldet.h"
#include "output.hpp"

namespace {

constexpr int kExUsage = 64;   // EX_USAGE, main.swift:40

void usage(FILE *to)
{
    std::fprintf(to,
                 "Usage: syllable-detector-cli -n <net> [-a <audio>]... [-d <seconds>] [--device <k>] [--chunk <frames>] [--format <shortest|swift4>] [--resample <linear|sinc>] [--resample-quality <Z,beta,rolloff>] [--simulate <out.wav>] [--simulate-output <k>] [--levels <out.tsv>] [--levels-buffer <L>] [--levels-period <seconds>] [--ttl <out.wav>] [--ttl-mux] [--ttl-width <seconds>] [--ttl-steps <n>] [--ttl-buffer <L>] [--ttl-latency <seconds>] [--ttl-onsets <out.tsv>] [--simulate-dir <dir>] [--ttl-dir <dir>] [--ttl-onsets-dir <dir>] [--batch] [--batch-rows <N>] [--batch-bytes <B>] [--score <labels.tsv> --score-out <table.tsv>] [--score-thresholds <lo:hi:n>] [--score-tolerance <seconds>] [--score-cost <c>] [--score-output <k>] [--align-dir <dir>] [--align <columns|outputs|samples>] [--align-at <detections|labels>] [--align-before <units>] [--align-after <units>] [--match <template.npy> --match-out <matches.tsv>]... [--match-threshold <v>]... [--match-separation <seconds>] [--match-anchor <frame>] [--match-ragged] [--train <labels.tsv> --train-out <net.txt>] [--train-steps <n>] [--train-rate <lr>] [--train-width <seconds>] [--train-seed <s>] [--train-fit-map] [--train-output <k>] [--train-log <log.tsv>] [--probe]\n"
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
                 "      --match <template.npy>:\n      Also find the occurrences of one exemplar in every track's spectrogram columns: a NumPy file of a little-endian float32 or float64 array [frames][bins] in C order, the bins those of the network's band (a window --align-dir writes, or sum.npy / count.npy). A position's score is the cosine between the template and the columns from there on; a match is a score at or above the threshold that nothing within the separation exceeds (the earlier of two equal ones). One network only. Needs --match-out. A file [exemplars][frames][bins] holds several exemplars of one syllable: a position's score is the greatest of theirs. Given several times (16 at most, 64 exemplars in all, every file the same frames and bins), the i-th --match is syllable class i and writes to the i-th --match-out, all classes in one pass; classes do not suppress each other. (A repeated --match used to replace the one before it.)\n"
                 "      --match-out <matches.tsv>:\n      Where --match writes its matches (given as many times as --match, in its order): lines of file, track and sample, tab separated, as --score reads them (the file as -a names it, the sample of the template's anchor frame at the network's rate), in command-line order, then track, then sample. With or without --batch, the same bytes.\n"
                 "      --match-threshold <v>:\n      The least score of a match (default 0.77): once for all classes, or as many times as --match, in its order.\n"
                 "      --match-separation <seconds>:\n      No two matches of a track are closer than this (default: the template's length; at most 4096 frames): once for all classes, or as many times as --match, in its order.\n"
                 "      --match-anchor <frame>:\n      The template's frame whose sample a match names (default: its last): once for all classes (a frame of the shortest template), or as many times as --match, in its order.\n"
                 "      --match-ragged:\n      The --match files may differ in their frame counts (without it that is an error): the classes are matched in one pass all the same, lined up at their --match-anchor frames. Files that all share their frame count write what they write without it.\n"
                 "      --train <labels.tsv>:\n      Under --batch, also train the (one) network on the batch's recordings: lines of file, track and sample as --score reads and --match-out writes them, the labelled samples of one output. An evaluation within --train-width of a label is a positive, every other a negative; the two classes weigh a half each. Adam on the mean squared error, full batch, on the GPU. The detections printed are those of the network as given. All audio files must go through one batch: otherwise nothing is trained or written. Where the network cannot be written the exit status is 1 at least. Needs --train-out.\n"
                 "      --train-out <net.txt>:\n      Where --train writes the trained network, in the text format -n reads.\n"
                 "      --train-steps <n>:\n      Steps of the optimiser (default 200).\n"
                 "      --train-rate <lr>:\n      The optimiser's learning rate (default 0.01).\n"
                 "      --train-width <seconds>:\n      An evaluation this close to a label is a positive (default: one hop of the spectrogram).\n"
                 "      --train-seed <s>:\n      Start from weights drawn from this seed instead of the network file's own.\n"
                 "      --train-fit-map:\n      Refit the network's first mapminmax input function to the batch's columns before training, as the MATLAB training code does.\n"
                 "      --train-output <k>:\n      The network output the labels belong to (default 0).\n"
                 "      --train-log <log.tsv>:\n      Also write the mean loss in front of every step, one line a step (step, loss; tab separated) behind a first line, # positives <n> negatives <n>.\n"
                 "      --probe:\n      Only print what the audio files contain; does not touch the GPU.\n"
                 "The command line will write a comma-separated list of detection events (when the network has at least one output above threshold) to standard out. For example, it might output:\n"
                 "\n\t0,1593298,36.1292063492063,0.918557\n\n"
                 "The columns are:\n"
                 "1. The track or channel number from the audio file (starting with 0).\n"
                 "2. The sample number from the audio when detection occurred.\n"
                 "3. The timestamp from the audio when detection occurred.\n"
                 "4. The first neural network output. Note that there may be additional columns for additional outputs.\n");
}

// a usage error: the message (none: only the text), the usage text, EX_USAGE
int fail(const std::string &message)
{
    if (!message.empty()) std::fprintf(stderr, "%s\n", message.c_str());
    usage(stdout);
    return kExUsage;
}

// --levels: the two meters of every row (Processor.swift:111-113, :138, :158-184) over the recording, as the 0.1 s timer of
// ViewControllerProcessor.swift:57 would have read them
struct LevelsOpt {
    std::string path;                                      // empty: none
    int buffer = 32;                                       // AudioInterface.swift:342, :474
    double period = 0.1;
};

// the buffers of a reading: the period in whole buffers, at least one
int64_t levels_period_buffers(const LevelsOpt &levels, double rate)
{
    const double per = levels.period * rate / (double)levels.buffer;
    return per >= 1.0 ? (per < 9e18 ? (int64_t)per : INT64_MAX) : 1;
}

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
    void make() const                                      // (a directory that cannot be made: the writes fail, and cost what they cost)
    {
        std::error_code ec;
        for (const std::string *d : {&simulate, &ttl, &onsets, &levels})
            if (!d->empty()) std::filesystem::create_directories(*d, ec);
    }
};

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

// --match: template matching (syldet_matcher_bank_*): the occurrences of exemplars [frames][bins] in the columns of every track of every
// file, written as the labels --score reads; the i-th --match (a file [exemplars][frames][bins]: several exemplars) is class i and
// writes the i-th --match-out.  The scores do not depend on where a track lies in a bank, so the file is the same
// bytes with and without --batch.  With --match-ragged, files of different frame counts make a ragged bank (syldet_matcher_bank_create_ragged): a class's
// templates share the file's length, the classes are lined up at their anchors.
struct MatchOpt {
    std::vector<std::string> paths, out_paths;             // a class each, in command-line order
    std::vector<double> thresholds;                        // none: 0.77; one: every class's; else a class each
    std::vector<double> separations;                       // in seconds; none: each class's own length; one: every class's; else a class each
    std::vector<long> anchors;                             // none: each class's last frame; one: every class's; else a class each
    bool ragged = false;                                   // --match-ragged: the files may differ in their frame counts
};

// --train: training (syldet_trainer_*, syldet_train_fit_device): the network of -n trained on the recordings of the one batch against
// labelled samples, and written in the text format.  Standard output is that of the run without it.
struct TrainOpt {
    std::string labels_path, out_path, log_path;           // empty: none
    long steps = 200;
    double rate = 0.01, width = -1.0;                       // the half width in seconds; < 0: one hop
    unsigned long long seed = 0;
    bool has_seed = false, fit_map = false;
    int output = 0;
};

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

// --score: threshold calibration (syldet_scorer_*): every track of every batched file scored against its labelled samples for
// a grid of candidate thresholds, on the outputs the batch leaves on the device.  The batches' tables add up on the host.
struct ScoreOpt {
    std::string labels_path, out_path;
    double lo = 0.0, hi = 1.0, tolerance = 0.02, cost = 1.0;
    long n = 101;
    int output = 0;
};

struct Options {
    std::vector<std::string> net, audio;
    double debounce = 0.0;                                  // (given: a number; "-d x" is no debounce)
    int device = 0;
    int64_t chunk = 8192;
    bool probe = false;
    std::string simulate;                                   // --simulate <out.wav>: see process_file
    int simulate_output = 0;
    ResampleOpt conv;
    LevelsOpt levels;
    TtlOpt ttl;
    BatchOpt batch;
    TrackDirs dirs;
    ScoreOpt score;
    AlignOpt align;
    MatchOpt match;
    TrainOpt train;
    std::set<std::string> given;                            // the options that were given, by their long names
    bool has(const char *name) const { return given.count(name) != 0; }
    bool any_of(std::initializer_list<const char *> names) const
    {
        for (const char *n : names)
            if (has(n)) return true;
        return false;
    }
};

// a whole-string integer from lo to hi, a power of two where asked
template <class T>
bool integer(const char *v, long long lo, long long hi, T &to, bool power_of_two = false)
{
    char *end = nullptr;
    const long long k = std::strtoll(v, &end, 10);
    if (end == v || *end != 0 || k < lo || k > hi || (power_of_two && (k & (k - 1)) != 0)) return false;
    to = (T)k;
    return true;
}

// a whole-string double that ok() takes
template <class Ok>
bool real(const char *v, double &to, Ok ok)
{
    char *end = nullptr;
    const double x = std::strtod(v, &end);
    if (end == v || *end != 0 || !ok(x)) return false;
    to = x;
    return true;
}

// lo:hi:n, the grid lo + (hi - lo) i / (n - 1)
bool score_grid(const std::string &v, ScoreOpt &score)
{
    const size_t c1 = v.find(':'), c2 = c1 == std::string::npos ? c1 : v.find(':', c1 + 1);
    const std::string lo = v.substr(0, c1), hi = c2 == std::string::npos ? "" : v.substr(c1 + 1, c2 - c1 - 1), n = c2 == std::string::npos ? "" : v.substr(c2 + 1);
    const auto number_of = [](double x) { return !std::isnan(x); };
    return !lo.empty() && !hi.empty() && !n.empty() && real(lo.c_str(), score.lo, number_of) && real(hi.c_str(), score.hi, number_of) &&
           integer(n.c_str(), 1, SYLDET_SCORE_MAX_THRESHOLDS, score.n);
}

// Z,beta,rolloff: three numbers, nothing else, inside the converter's ranges (syldet_sinc_taps knows Z's and rolloff's)
bool resample_quality(const char *v, ResampleOpt &conv)
{
    char *e1 = nullptr, *e2 = nullptr, *e3 = nullptr;
    const long z = std::strtol(v, &e1, 10);
    const double b = e1 != v && *e1 == ',' ? std::strtod(e1 + 1, &e2) : 0.0;
    const double r = e2 && e2 != e1 + 1 && *e2 == ',' ? std::strtod(e2 + 1, &e3) : 0.0;
    if (!e3 || e3 == e2 + 1 || *e3 != 0 || z < 4 || z > 64 || !(b >= 0.0 && b <= 20.0) || !(r > 0.0 && r <= 1.0)) return false;
    conv.zero_crossings = (int32_t)z; conv.beta = b; conv.rolloff = r;
    return true;
}

// Reads the options into o.  -1: go on; otherwise the status to exit with (a usage error, or --format-line's 0).
int parse_options(int argc, char **argv, Options &o)
{
    syldet_sinc_defaults(&o.conv.zero_crossings, &o.conv.beta, &o.conv.rolloff);
    const auto positive = [](double x) { return x > 0.0 && !(x > 1e15); };
    const auto zero_or_more = [](double x) { return x >= 0.0 && !(x > 1e15); };
    const auto finite_zero_or_more = [](double x) { return x >= 0.0 && !std::isinf(x); };
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        a = a == "-n" ? "--net" : a == "-a" ? "--audio" : a == "-d" ? "--debounce" : a;
        std::string v;                                      // the option's value, by text() for those that take words
        const auto value = [&]() -> const char * {
            if (i + 1 >= argc) {
                std::fprintf(stderr, "Missing value for %s.\n", a.c_str());
                usage(stdout);
                std::exit(kExUsage);
            }
            return argv[++i];
        };
        const auto text = [&]() -> const std::string & { return v = value(); };
        o.given.insert(a);
        if (a == "--net") o.net.push_back(value());
        else if (a == "--audio") o.audio.push_back(value());
        else if (a == "--debounce") { if (!real(value(), o.debounce, [](double) { return true; })) o.given.erase(a); }   // Double.init(String): nil (no debounce) when not a number
        else if (a == "--device") o.device = std::atoi(value());
        else if (a == "--chunk") o.chunk = std::atoll(value());
        else if (a == "--probe") o.probe = true;
        else if (a == "--batch") o.batch.on = true;
        else if (a == "--batch-rows") { if (!integer(value(), 1, 65535, o.batch.rows)) return fail("--batch-rows takes a number of rows from 1 to 65535."); }
        else if (a == "--batch-bytes") { if (!integer(value(), 1, INT64_MAX, o.batch.bytes)) return fail("--batch-bytes takes a number of bytes, 1 or more."); }
        else if (a == "--score") o.score.labels_path = value();
        else if (a == "--score-out") o.score.out_path = value();
        else if (a == "--score-thresholds") { if (!score_grid(value(), o.score)) return fail("--score-thresholds takes lo:hi:n, two numbers and a count from 1 to " + std::to_string(SYLDET_SCORE_MAX_THRESHOLDS) + "."); }
        else if (a == "--score-tolerance") { if (!real(value(), o.score.tolerance, finite_zero_or_more)) return fail(a + " takes a number, 0 or more."); }
        else if (a == "--score-cost") { if (!real(value(), o.score.cost, finite_zero_or_more)) return fail(a + " takes a number, 0 or more."); }
        else if (a == "--score-output") { if (!integer(value(), 0, 65535, o.score.output)) return fail("--score-output takes the number of a network output, 0 or more."); }
        else if (a == "--align-dir") o.align.dir = value();
        else if (a == "--align") {
            if (text() != "columns" && v != "outputs" && v != "samples") return fail("--align takes columns, outputs or samples.");
            o.align.source = v == "columns" ? SYLDET_ALIGN_COLUMNS : v == "outputs" ? SYLDET_ALIGN_OUTPUTS : SYLDET_ALIGN_SAMPLES;
        } else if (a == "--align-at") {
            if (text() != "detections" && v != "labels") return fail("--align-at takes detections or labels.");
            o.align.at_labels = v == "labels";
        }
        else if (a == "--align-before") { if (!integer(value(), 0, SYLDET_ALIGN_MAX_WINDOW, o.align.before)) return fail("--align-before and --align-after take a number of units, 0 or more."); }
        else if (a == "--align-after") { if (!integer(value(), 0, SYLDET_ALIGN_MAX_WINDOW, o.align.after)) return fail("--align-before and --align-after take a number of units, 0 or more."); }
        else if (a == "--match") o.match.paths.push_back(value());
        else if (a == "--match-out") o.match.out_paths.push_back(value());
        else if (a == "--match-ragged") o.match.ragged = true;
        else if (a == "--match-threshold") { double v = 0.0; if (!real(value(), v, [](double x) { return !std::isnan(x); })) return fail("--match-threshold takes a number."); o.match.thresholds.push_back(v); }
        else if (a == "--match-separation") { double v = 0.0; if (!real(value(), v, finite_zero_or_more)) return fail("--match-separation takes a number of seconds, 0 or more."); o.match.separations.push_back(v); }
        else if (a == "--match-anchor") { long v = 0; if (!integer(value(), 0, SYLDET_MATCH_MAX_TEMPLATE - 1, v)) return fail("--match-anchor takes a frame of the template, 0 or more."); o.match.anchors.push_back(v); }
        else if (a == "--train") o.train.labels_path = value();
        else if (a == "--train-out") o.train.out_path = value();
        else if (a == "--train-log") o.train.log_path = value();
        else if (a == "--train-steps") { if (!integer(value(), 0, 1L << 24, o.train.steps)) return fail("--train-steps takes a number of steps, 0 or more."); }
        else if (a == "--train-rate") { if (!real(value(), o.train.rate, [](double x) { return x > 0.0 && !std::isinf(x); })) return fail("--train-rate takes a positive number."); }
        else if (a == "--train-width") { if (!real(value(), o.train.width, finite_zero_or_more)) return fail("--train-width takes a number of seconds, 0 or more."); }
        else if (a == "--train-seed") {
            long long seed = 0;
            if (!integer(value(), 0, INT64_MAX, seed)) return fail("--train-seed takes a whole number, 0 or more.");
            o.train.seed = (unsigned long long)seed;
            o.train.has_seed = true;
        }
        else if (a == "--train-fit-map") o.train.fit_map = true;
        else if (a == "--train-output") { if (!integer(value(), 0, 65535, o.train.output)) return fail("--train-output takes the number of a network output, 0 or more."); }
        else if (a == "--resample") {
            if (text() != "linear" && v != "sinc") return fail("--resample takes linear or sinc.");
            o.conv.sinc = v == "sinc";
        }
        else if (a == "--resample-quality") { if (!resample_quality(value(), o.conv)) return fail("--resample-quality takes Z,beta,rolloff: 4 to 64 zero crossings, beta from 0 to 20, a rolloff above 0 and at most 1."); }
        else if (a == "--simulate") o.simulate = value();
        else if (a == "--simulate-dir") o.dirs.simulate = value();
        else if (a == "--levels-dir") o.dirs.levels = value();
        else if (a == "--ttl-dir") o.dirs.ttl = value();
        else if (a == "--ttl-onsets-dir") o.dirs.onsets = value();
        else if (a == "--simulate-output") { if (!integer(value(), 0, 0x7fffffffL, o.simulate_output)) return fail("--simulate-output takes an output number (0, 1, ...)."); }
        else if (a == "--levels") o.levels.path = value();
        else if (a == "--levels-buffer") { if (!integer(value(), 8, 4096, o.levels.buffer, true)) return fail("--levels-buffer takes a power of two from 8 to 4096."); }
        else if (a == "--levels-period") { if (!real(value(), o.levels.period, positive)) return fail("--levels-period takes a positive number of seconds."); }
        else if (a == "--ttl") o.ttl.path = value();
        else if (a == "--ttl-onsets") o.ttl.onsets = value();
        else if (a == "--ttl-mux") o.ttl.mux = true;
        else if (a == "--ttl-width") { if (!real(value(), o.ttl.width, positive)) return fail("--ttl-width takes a positive number of seconds."); }
        else if (a == "--ttl-latency") { if (!real(value(), o.ttl.latency, zero_or_more)) return fail("--ttl-latency takes a number of seconds, 0 or more."); }
        else if (a == "--ttl-steps") { if (!integer(value(), 1, 1L << 24, o.ttl.steps)) return fail("--ttl-steps takes a number of buffers, 1 or more."); }
        else if (a == "--ttl-buffer") { if (!integer(value(), 8, 4096, o.ttl.buffer, true)) return fail("--ttl-buffer takes a power of two from 8 to 4096."); }
        else if (a == "--format") {
            if (text() != "shortest" && v != "swift4") return fail("");
            g_swift4 = v == "swift4";
        } else if (a == "--format-line") {
            if (i + 3 >= argc) return fail("");
            format_line(argc - i - 1, argv + i + 1);
            return 0;
        }
        else return fail("");                              // -h, --help and anything unknown: usage text, EX_USAGE (main.swift:27-41)
    }
    return -1;
}

// two audio files of one name (or of a name in taken) cannot both be written under it: the name, or empty
std::string name_given_twice(const std::vector<std::string> &audio, std::set<std::string> taken)
{
    for (const std::string &p : audio)
        if (!taken.insert(TrackDirs::name_of(p)).second) return TrackDirs::name_of(p);
    return std::string();
}

// The checks that need only the options, in the order in which they are reported.  0, or the usage error.
int check_options(const Options &o)
{
    const bool one_file = o.audio.size() == 1;
    if (o.has("--resample-quality") && !o.conv.sinc) return fail("--resample-quality needs --resample sinc.");
    // the Simulator takes one recording (simulateNetwork(_:withAudio:writeTo:), ViewControllerSimulator.swift:135)
    if (o.has("--simulate") && (!one_file || o.simulate.empty())) return fail("--simulate writes the track of exactly one audio file (-a).");
    if ((o.has("--simulate-dir") && o.dirs.simulate.empty()) || (o.has("--ttl-dir") && o.dirs.ttl.empty()) || (o.has("--ttl-onsets-dir") && o.dirs.onsets.empty()))
        return fail("--simulate-dir, --ttl-dir and --ttl-onsets-dir take the name of a directory.");
    if ((o.has("--simulate") && o.has("--simulate-dir")) || (o.has("--ttl") && o.has("--ttl-dir")) || (o.has("--ttl-onsets") && o.has("--ttl-onsets-dir")))
        return fail("--simulate-dir, --ttl-dir and --ttl-onsets-dir write what --simulate, --ttl and --ttl-onsets write, for every audio file: give the one or the other.");
    if (o.has("--levels-dir") && o.dirs.levels.empty()) return fail("--levels-dir takes the name of a directory.");
    if (o.has("--levels") && o.has("--levels-dir")) return fail("--levels-dir writes what --levels writes, for every audio file: give the one or the other.");
    if (o.has("--align-dir") && o.align.dir.empty()) return fail("--align-dir takes the name of a directory.");
    if (o.any_of({"--align", "--align-at", "--align-before", "--align-after"}) && !o.has("--align-dir"))
        return fail("--align, --align-at, --align-before and --align-after need --align-dir <dir>.");
    if (o.align.at_labels && !o.has("--score")) return fail("--align-at labels needs --score <labels.tsv>.");
    if (o.has("--match-ragged") && !o.has("--match")) return fail("--match-ragged needs --match <template.npy>.");
    if (o.any_of({"--match-out", "--match-threshold", "--match-separation", "--match-anchor"}) && !o.has("--match"))
        return fail("--match-out, --match-threshold, --match-separation and --match-anchor need --match <template.npy>.");
    if (o.has("--match") && o.match.out_paths.empty()) return fail("--match <template.npy> needs --match-out <matches.tsv>.");
    if (o.has("--match") && o.match.paths.size() != o.match.out_paths.size())
        return fail("--match and --match-out are given equally often: the i-th --match is class i and writes the i-th --match-out.");
    if (o.match.paths.size() > SYLDET_MATCH_MAX_CLASSES) return fail("--match may be given " + std::to_string(SYLDET_MATCH_MAX_CLASSES) + " times at most.");
    if (o.match.thresholds.size() > 1 && o.match.thresholds.size() != o.match.paths.size())
        return fail("--match-threshold is given once for all classes, or as many times as --match.");
    if (o.match.separations.size() > 1 && o.match.separations.size() != o.match.paths.size())
        return fail("--match-separation is given once for all classes, or as many times as --match.");
    if (o.match.anchors.size() > 1 && o.match.anchors.size() != o.match.paths.size())
        return fail("--match-anchor is given once for all classes, or as many times as --match.");
    if (o.any_of({"--train-out", "--train-steps", "--train-rate", "--train-width", "--train-seed", "--train-fit-map", "--train-output", "--train-log"}) && !o.has("--train"))
        return fail("--train-out, --train-steps, --train-rate, --train-width, --train-seed, --train-fit-map, --train-output and --train-log need --train <labels.tsv>.");
    // the trainer's detectors are the recordings of a batch
    if (o.has("--train") && !o.batch.on) return fail("--train needs --batch.");
    if (o.has("--train") && (o.train.labels_path.empty() || o.train.out_path.empty())) return fail("--train <labels.tsv> needs --train-out <net.txt>.");
    if (o.has("--train") && o.net.size() > 1) return fail("--train takes one network (-n).");
    // (what needs the loaded network -- one the trainer does not take, --train-output beyond its outputs, --train-fit-map without a
    // mapminmax -- is a usage error of train_begin, cli/train.hpp, reported behind these and before the GPU is opened)
    std::string twice;
    // every audio file's windows go under its own name, beside the three stack files
    if (o.has("--align-dir") && !(twice = name_given_twice(o.audio, {"count", "sum", "sumsq"})).empty())
        return fail("--align-dir names its files after the audio files (and count, sum, sumsq): two of those are called " + twice + ".");
    // every audio file's products go under its own name
    if ((o.dirs.any() || o.has("--levels-dir")) && !(twice = name_given_twice(o.audio, {})).empty())
        return fail("--simulate-dir, --ttl-dir, --ttl-onsets-dir and --levels-dir name their files after the audio files: two of those are called " + twice + ".");
    if (o.ttl.mux && o.batch.on) return fail("--ttl-mux is not available under --batch.");
    if (o.has("--simulate-output") && !o.has("--simulate") && !o.has("--simulate-dir")) return fail("--simulate-output needs --simulate <out.wav> or --simulate-dir <dir>.");
    // one table, one recording
    if (o.has("--levels") && (!one_file || o.levels.path.empty())) return fail("--levels writes the readings of exactly one audio file (-a).");
    if (o.any_of({"--levels-buffer", "--levels-period"}) && !o.has("--levels") && !o.has("--levels-dir"))
        return fail("--levels-buffer and --levels-period need --levels <out.tsv> or --levels-dir <dir>.");
    // one rig, one recording
    if ((o.has("--ttl") && (!one_file || o.ttl.path.empty())) || (o.has("--ttl-onsets") && (!one_file || o.ttl.onsets.empty())))
        return fail("--ttl and --ttl-onsets write the triggers of exactly one audio file (-a).");
    if (o.ttl.mux && !o.has("--ttl") && !o.has("--ttl-dir")) return fail("--ttl-mux needs --ttl <out.wav> or --ttl-dir <dir>.");
    if (o.any_of({"--ttl-width", "--ttl-steps", "--ttl-buffer", "--ttl-latency"}) && !o.any_of({"--ttl", "--ttl-onsets", "--ttl-dir", "--ttl-onsets-dir"}))
        return fail("--ttl-width, --ttl-steps, --ttl-buffer and --ttl-latency need --ttl <out.wav>, --ttl-onsets <out.tsv>, --ttl-dir <dir> or --ttl-onsets-dir <dir>.");
    if (o.has("--ttl-width") && o.has("--ttl-steps")) return fail("--ttl-width and --ttl-steps both set the pulse's width: give one.");
    if (o.any_of({"--batch-rows", "--batch-bytes"}) && !o.batch.on) return fail("--batch-rows and --batch-bytes need --batch.");
    // (one table, one file; a batch's tables go to --levels-dir)
    if (o.batch.on && o.has("--levels")) return fail("--levels is not available under --batch: it takes exactly one file and a bank of its own.");
    // those name one file; under --batch every file's tracks go to a directory
    if (o.batch.on && o.any_of({"--simulate", "--ttl", "--ttl-onsets"}))
        return fail("--batch runs many files through one bank; --simulate, --ttl and --ttl-onsets take exactly one file: give --simulate-dir, --ttl-dir and --ttl-onsets-dir instead.");
    const bool score_option = o.any_of({"--score-out", "--score-thresholds", "--score-tolerance", "--score-cost", "--score-output"});
    const bool labels_only = o.has("--score") && !o.batch.on && o.align.at_labels && !score_option;   // --score as the file of --align-at labels
    // the scorer's detectors are the recordings of a batch
    if (o.has("--score") && !o.batch.on && !labels_only) return fail("--score needs --batch.");
    if (score_option && !o.has("--score")) return fail("--score-out, --score-thresholds, --score-tolerance, --score-cost and --score-output need --score <labels.tsv>.");
    if (o.has("--score") && !labels_only && (o.score.labels_path.empty() || o.score.out_path.empty())) return fail("--score <labels.tsv> needs --score-out <table.tsv>.");
    return 0;
}

}  // namespace
