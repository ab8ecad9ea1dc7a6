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
// --match writes the occurrences of an exemplar in every track's columns as the labels --score reads; given several times, each is a
// syllable class of one or more exemplars with a file of its own, all matched in one pass (syldet_matcher_bank_*).
// --train trains the network on the one batch's recordings against such labels and writes it in the text format (syldet_trainer_*,
// syldet_train_fit_device, syldet_config_save_text).
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

#include "batch.hpp"

namespace {

// the configurations, freed on every way out
struct Configs {
    std::vector<syldet_config_t *> v;
    ~Configs() { for (syldet_config_t *c : v) syldet_config_free(c); }
};

int probe_files(const std::vector<std::string> &audio)
{
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

// The checks that need the loaded networks, in the order in which they are reported, and what --score and --align-dir run with
// (all before the GPU is opened).  0, or the usage error.
int check_networks(const Options &o, const std::vector<syldet_config_t *> &cfgs, ScoreRun &scoring, AlignRun &aligning)
{
    const double rate = cfgs[0]->sampling_rate;
    if (o.has("--simulate") || o.has("--simulate-dir"))
        for (const syldet_config_t *c : cfgs)
            if (o.simulate_output >= c->n_thresholds) return fail("--simulate-output " + std::to_string(o.simulate_output) + ": the network has " + std::to_string(c->n_thresholds) + " output(s).");
    if (o.ttl.any() || o.has("--ttl-dir") || o.has("--ttl-onsets-dir")) {
        const int64_t N = o.ttl.width_samples(rate), lat = o.ttl.latency_samples(rate);
        if (N < 1) return fail("--ttl-width: shorter than one sample at " + swift_number(rate) + " Hz.");
        if (N > (1ll << 24) || lat > (1ll << 24)) return fail("The pulse's width and --ttl-latency may be 16777216 samples at most.");
    }
    if (o.has("--score")) {
        const double tol = o.score.tolerance * rate;
        if (!(tol <= (double)SYLDET_SCORE_MAX_TOLERANCE)) return fail("--score-tolerance may be " + std::to_string(SYLDET_SCORE_MAX_TOLERANCE) + " samples at most.");
        for (const syldet_config_t *c : cfgs)
            if (o.score.output >= c->n_thresholds) return fail("--score-output " + std::to_string(o.score.output) + ": the network has " + std::to_string(c->n_thresholds) + " output(s).");
        scoring.tolerance = (int64_t)tol;
        scoring.output = o.score.output;
        for (long i = 0; i < o.score.n; i++) scoring.thresholds.push_back(o.score.n > 1 ? o.score.lo + (o.score.hi - o.score.lo) * (double)i / (double)(o.score.n - 1) : o.score.lo);
        scoring.totals.assign((size_t)o.score.n * SYLDET_SCORE_COLUMNS, 0);
    }
    return o.has("--align-dir") ? align_begin(aligning, o.align, cfgs, &scoring.labels) : 0;
}

}  // namespace

int main(int argc, char **argv)
{
    Options o;
    if (const int rc = parse_options(argc, argv, o); rc >= 0) return rc;
    if (o.probe) return probe_files(o.audio);
    if (o.net.empty()) return fail("");                     // the option is .required() in the reference (main.swift:21)
    if (const int rc = check_options(o)) return rc;
    ScoreRun scoring;
    std::string err;
    if (o.has("--score") && !read_labels(o.score.labels_path, scoring, err)) return fail("--score: " + err + ".");
    Configs configs;
    for (const std::string &n : o.net) {
        syldet_config_t *cfg = nullptr;
        if (int st = syldet_config_load_text(n.c_str(), &cfg)) {
            std::fprintf(stderr, "Unable to load the network configuration: %s: %s\n", syldet_strerror(st), syldet_last_error());
            return 1;
        }
        cfg->rule = SYLDET_RULE_ANY;                        // any output above its threshold, TrackDetector.swift:72-77
        configs.v.push_back(cfg);
    }
    AlignRun aligning;
    if (const int rc = check_networks(o, configs.v, scoring, aligning)) return rc;
    MatchRun matching;
    if (o.has("--match"))
        if (const int rc = match_begin(matching, o.match, configs.v)) return rc;
    TrainRun training;
    if (o.has("--train"))
        if (const int rc = train_begin(training, o.train, configs.v)) return rc;
    const Run run{o, configs.v, o.has("--debounce") ? o.debounce : 0.0, o.has("--score") ? &scoring : nullptr, o.has("--align-dir") ? &aligning : nullptr,
                  o.has("--match") ? &matching : nullptr, o.has("--train") ? &training : nullptr};
    int rc = 0;
    o.dirs.make();
    if (o.batch.on) {
        rc = process_batched(run);
        // the table last, and only a whole one; standard output and the status are those of the run without --score
        if (run.score && (scoring.failed || !write_score_table(o.score, scoring)) && rc == 0) rc = 1;
    } else {
        for (const std::string &p : o.audio) {
            if (o.audio.size() > 1) std::printf("%s\n", p.c_str());   // main.swift:122-124
            std::fflush(stdout);
            fold_status(rc, process_file(run, p, products_of(o, p)));
        }
    }
    if (run.align && !align_finish(aligning) && rc == 0) rc = 1;
    if (run.match && !match_finish(matching) && rc == 0) rc = 1;
    if (run.train && !train_finish(training, configs.v[0]) && rc == 0) rc = 1;
    return rc;
}
