// --train: the labels and what a run keeps (see TrainOpt), the training of one batch's recordings on the device, and the network and
// the log written at the end.
#pragma once

#include <hip/hip_runtime.h>

#include "match.hpp"

namespace {

struct TrainRun {
    TrainOpt opt;
    ScoreRun labels;                                        // (the labels file is --score's: only .labels is used)
    int64_t half_width = 0;                                 // samples
    int64_t n_params = 0;
    int I = 0, H = 0, O = 0;
    int batches = 0;                                        // batches the run has seen: training takes exactly one
    bool several = false, outside = false;                  // the files pass --batch-bytes; a file does not go through the bank
    bool failed = false, trained = false;
    int64_t n_pos = 0, n_neg = 0;
    std::vector<float> params, x_offsets, gains;            // what comes back: the parameters, the fitted map (empty: the network's own)
    std::vector<double> history;
};

// The labels, and the options in the network's units (all before the GPU is opened).  0, or the usage error.
int train_begin(TrainRun &run, const TrainOpt &opt, const std::vector<syldet_config_t *> &cfgs)
{
    run.opt = opt;
    const syldet_config_t *c = cfgs[0];
    syldet_geometry_t g;
    if (const int st = syldet_config_geometry(c, &g)) return fail(std::string("Unable to use the network configuration: ") + syldet_strerror(st) + ": " + syldet_last_error());
    if (syldet_train_param_count(c, &run.n_params)) return fail(std::string("--train: the trainer does not take this network: ") + syldet_last_error() + ".");
    run.I = c->layers[0].inputs;
    run.H = c->layers[0].outputs;
    run.O = c->layers[1].outputs;
    if (run.H > SYLDET_TRAIN_MAX_HIDDEN || run.O > SYLDET_TRAIN_MAX_OUTPUTS)
        return fail("--train: the trainer does not take this network: up to " + std::to_string(SYLDET_TRAIN_MAX_HIDDEN) + " hidden units and " +
                    std::to_string(SYLDET_TRAIN_MAX_OUTPUTS) + " outputs.");
    if (opt.output >= run.O) return fail("--train-output " + std::to_string(opt.output) + ": the network has " + std::to_string(run.O) + " output(s).");
    if (opt.fit_map) {
        bool has = false;
        for (int k = 0; k < c->n_input_fns; k++) has = has || c->input_fns[k].kind == SYLDET_FN_MAPMINMAX;
        if (!has) return fail("--train-fit-map: the network has no mapminmax input function.");
    }
    const double hw = opt.width < 0.0 ? (double)g.hop : opt.width * c->sampling_rate;
    if (!(hw <= 1099511627776.0)) return fail("--train-width may be 1099511627776 samples at most.");
    run.half_width = (int64_t)hw;
    std::string err;
    if (!read_labels(opt.labels_path, run.labels, err)) return fail("--train: " + err + ".");
    return 0;
}

// One batch's recordings (r) from the fp32 rows the bank was fed: the rows' columns, targets and class weights from the labels, the
// input map from the columns' range (--train-fit-map), then the fit; one download of the parameters and the history.  names: every
// recording's file and track.  false: the device's or the library's refusal (a message is out).
bool train_bank(TrainRun &run, syldet_t *h, syldet_recordings_t *r, const syldet_config_t *cfg, const float *rows, int64_t row_samples, int64_t row_evals, int C,
                const std::vector<std::pair<std::string, int>> &names, hipStream_t stream)
{
    const int K = (int)names.size();
    const int64_t J = std::max<int64_t>(0, syldet_count_frames(h, row_samples));
    if (J <= 0 || row_evals <= 0 || K <= 0) {
        std::fprintf(stderr, "--train: no file of the batch is long enough for one evaluation.\n");
        return false;
    }
    syldet_geometry_t g;
    syldet_get_geometry(h, &g);
    // the labels in the recordings' order, all of output --train-output; the classes' sizes over the recordings' own evaluations
    std::vector<syldet_slot_t> slots((size_t)K);
    std::vector<int64_t> labels, begin{0};
    int st = syldet_recordings_slots(r, slots.data());
    run.n_pos = run.n_neg = 0;
    for (int k = 0; !st && k < K; k++) {
        const std::vector<int64_t> &mine = labels_of(run.labels.labels, names[(size_t)k].first, names[(size_t)k].second);
        labels.insert(labels.end(), mine.begin(), mine.end());
        begin.push_back((int64_t)labels.size());
        const int64_t n = slots[(size_t)k].n_evals;
        std::vector<float> t((size_t)std::max<int64_t>(n, 1)), w((size_t)std::max<int64_t>(n, 1));
        st = syldet_train_targets_host(mine.data(), (int64_t)mine.size(), nullptr, 1, run.half_width, 1.0f, 0.0f, g.first_index, g.hop, n, t.data(), w.data());
        for (int64_t e = 0; !st && e < n; e++) (w[(size_t)e] > 0.0f ? run.n_pos : run.n_neg)++;
    }
    if (!st && (run.n_pos == 0 || run.n_neg == 0)) {
        std::fprintf(stderr, "--train: the labels give %lld positive and %lld negative evaluations; both classes are needed.\n", (long long)run.n_pos, (long long)run.n_neg);
        return false;
    }
    const std::vector<int32_t> outs(labels.size(), (int32_t)run.opt.output);
    const int64_t P = run.n_params;
    syldet_trainer_t *t = nullptr;
    DevBuf d_cols, d_targets, d_weights, d_params, d_history, d_range, d_count;
    bool ok = true;
    if (!st) st = syldet_trainer_create(h, r, &t);
    if (!st) {
        ok = d_cols.alloc((size_t)C * (size_t)J * (size_t)g.bins * sizeof(float)) && d_targets.alloc((size_t)C * (size_t)row_evals * (size_t)run.O * sizeof(float)) &&
             d_weights.alloc((size_t)C * (size_t)row_evals * sizeof(float)) && d_params.alloc((size_t)P * sizeof(float)) &&
             d_history.alloc((size_t)std::max<long>(run.opt.steps, 1) * sizeof(double)) && d_range.alloc(2 * (size_t)run.I * sizeof(float)) && d_count.alloc(sizeof(int64_t));
        if (ok) st = syldet_spectrogram_device(h, rows, row_samples, row_samples, (float *)d_cols.p, stream);
        if (ok && !st)
            st = syldet_train_targets_device(t, labels.data(), begin.data(), outs.data(), run.half_width, (float)(0.5 / (double)run.n_pos), (float)(0.5 / (double)run.n_neg), row_evals,
                                             (float *)d_targets.p, (float *)d_weights.p, stream);
    }
    // the starting parameters: the network's own, or the seeded draw
    run.params.assign((size_t)P, 0.0f);
    if (ok && !st) {
        if (run.opt.has_seed) {
            st = syldet_train_init_host(run.opt.seed, run.I, run.H, run.O, run.params.data());
        } else {
            float *at = run.params.data();
            for (int l = 0; l < 2; l++) {
                const syldet_layer_t &L = cfg->layers[l];
                at = std::copy(L.weights, L.weights + (size_t)L.inputs * (size_t)L.outputs, at);
                at = std::copy(L.biases, L.biases + L.outputs, at);
            }
        }
        if (!st) ok = hipMemcpyAsync(d_params.p, run.params.data(), (size_t)P * sizeof(float), hipMemcpyHostToDevice, stream) == hipSuccess;
    }
    // --train-fit-map: the range of the chain in front of the map over every weighted evaluation, the map of that range, into the trainer
    if (ok && !st && run.opt.fit_map) {
        std::vector<float> range(2 * (size_t)run.I);
        int64_t count = 0;
        st = syldet_train_input_range_device(t, (const float *)d_cols.p, J, 0, (const float *)d_weights.p, row_evals, (float *)d_range.p, (int64_t *)d_count.p, stream);
        if (!st)
            ok = hipMemcpyAsync(range.data(), d_range.p, range.size() * sizeof(float), hipMemcpyDeviceToHost, stream) == hipSuccess &&
                 hipMemcpyAsync(&count, d_count.p, sizeof count, hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
        if (ok && !st && count == 0) {
            std::fprintf(stderr, "--train-fit-map: no evaluation has a whole, finite network input; the map cannot be fitted.\n");
            syldet_trainer_destroy(t);
            return false;
        }
        if (ok && !st) {
            run.x_offsets.assign((size_t)run.I, 0.0f);
            run.gains.assign((size_t)run.I, 0.0f);
            st = syldet_train_input_map_host(range.data(), run.I, run.x_offsets.data(), run.gains.data());
            if (!st) st = syldet_trainer_set_input_map(t, run.x_offsets.data(), run.gains.data(), -1.0f);
        }
    }
    run.history.assign((size_t)run.opt.steps, 0.0);
    if (ok && !st)
        st = syldet_train_fit_device(t, (const float *)d_cols.p, J, 0, (const float *)d_targets.p, (const float *)d_weights.p, row_evals, (float *)d_params.p, run.opt.steps,
                                     run.opt.rate, 0.9, 0.999, 1e-8, (double *)d_history.p, stream);
    if (ok && !st)
        ok = hipMemcpyAsync(run.params.data(), d_params.p, (size_t)P * sizeof(float), hipMemcpyDeviceToHost, stream) == hipSuccess &&
             (run.history.empty() || hipMemcpyAsync(run.history.data(), d_history.p, run.history.size() * sizeof(double), hipMemcpyDeviceToHost, stream) == hipSuccess) &&
             hipStreamSynchronize(stream) == hipSuccess;
    syldet_trainer_destroy(t);
    if (st) std::fprintf(stderr, "Unable to train the network: %s: %s\n", syldet_strerror(st), syldet_last_error());
    else if (!ok) std::fprintf(stderr, "Unable to train the network: %s\n", hipGetErrorString(hipGetLastError()));
    return ok && !st;
}

// the network and the log, behind the last audio file
bool train_finish(const TrainRun &run, const syldet_config_t *cfg)
{
    if (run.several || run.batches > 1 || run.outside) {
        std::fprintf(stderr, "--train: the audio files do not go through one batch (%s); a gradient over several batches is not available: raise --batch-bytes.\n",
                     run.outside ? "a file runs outside the bank" : "they pass --batch-bytes");
        return false;
    }
    if (run.failed || !run.trained) {
        if (!run.failed) std::fprintf(stderr, "--train: no batch was run; nothing is written.\n");
        return false;
    }
    syldet_config_t *made = nullptr;
    const bool fitted = !run.x_offsets.empty();
    int st = syldet_train_config_with(cfg, run.params.data(), run.n_params, fitted ? run.x_offsets.data() : nullptr, fitted ? run.gains.data() : nullptr, -1.0f, &made);
    if (!st) st = syldet_config_save_text(made, run.opt.out_path.c_str());
    syldet_config_free(made);
    if (st) {
        std::fprintf(stderr, "Unable to write %s: %s: %s\n", run.opt.out_path.c_str(), syldet_strerror(st), syldet_last_error());
        return false;
    }
    if (run.opt.log_path.empty()) return true;
    // LOG: "# positives <n> negatives <n>", then step<TAB>mean loss in front of that step, one line a step
    FILE *f = std::fopen(run.opt.log_path.c_str(), "wb");
    bool ok = f != nullptr;
    if (ok) ok = std::fprintf(f, "# positives %lld negatives %lld\n", (long long)run.n_pos, (long long)run.n_neg) > 0;
    for (size_t k = 0; ok && k < run.history.size(); k++) ok = std::fprintf(f, "%zu\t%.17g\n", k + 1, run.history[k]) > 0;
    if (f && std::fclose(f) != 0) ok = false;
    if (!ok) std::fprintf(stderr, "Unable to write %s.\n", run.opt.log_path.c_str());
    return ok;
}

}  // namespace
