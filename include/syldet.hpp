// syldet.hpp -- C++ mirror of the reference's Swift interface for this path, over the C ABI in
// syldet.h.  Header-only; links against libsyldet.so.
//
// The reference is compiled Swift (no Swift toolchain in the build image), so the host side above
// the C ABI is written in C++ with the reference's names, argument meaning and error behaviour:
//   SyllableDetectorConfig(fromTextFile:)  throws ParseError     Common/SyllableDetectorConfig.swift:170-277
//   SyllableDetector(config:)              fatalError on mismatch Common/SyllableDetector.swift:37-74
//   appendAudioData(_:withSamples:)                               :129-132
//   processNewValue() -> Bool                                     :153-217
//   lastOutputs / lastDetected / seenSyllable()                   :26-31, :220-230
//   ResamplerLinear(fromRate:toRate:).resampleVector / resampleArray  Common/Resampler.swift:20-76
// Swift's fatalError becomes syldetxx::FatalError (a std::runtime_error carrying the status);
// ParseError keeps its four kinds.  A detector here is one channel of a bank; `SyllableDetectorBank`
// is the batched form the MI355X engine is built around.
#pragma once

#include <algorithm>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "syldet.h"

namespace syldetxx {

struct FatalError : std::runtime_error {
    int status;
    FatalError(int st, const std::string &msg) : std::runtime_error(msg), status(st) {}
};

// SyllableDetectorConfig.ParseError, SyllableDetectorConfig.swift:50-55
struct ParseError : std::runtime_error {
    enum Kind { unableToOpenPath, missingValue, invalidValue, mismatchedLength } kind;
    ParseError(Kind k, const std::string &msg) : std::runtime_error(msg), kind(k) {}
};

inline void check(int status)
{
    if (status >= 0) return;
    const std::string msg = std::string(syldet_strerror(status)) + ": " + syldet_last_error();
    switch (status) {
    case SYLDET_ERR_PARSE_OPEN: throw ParseError(ParseError::unableToOpenPath, msg);
    case SYLDET_ERR_PARSE_MISSING: throw ParseError(ParseError::missingValue, msg);
    case SYLDET_ERR_PARSE_INVALID: throw ParseError(ParseError::invalidValue, msg);
    case SYLDET_ERR_PARSE_LENGTH: throw ParseError(ParseError::mismatchedLength, msg);
    default: throw FatalError(status, msg);
    }
}

// SyllableDetectorConfig (struct, SyllableDetectorConfig.swift:11-45): same stored fields.
class SyllableDetectorConfig {
public:
    explicit SyllableDetectorConfig(const std::string &fromTextFile) { check(syldet_config_load_text(fromTextFile.c_str(), &cfg_)); }
    ~SyllableDetectorConfig() { syldet_config_free(cfg_); }
    SyllableDetectorConfig(const SyllableDetectorConfig &) = delete;
    SyllableDetectorConfig &operator=(const SyllableDetectorConfig &) = delete;

    double samplingRate() const { return cfg_->sampling_rate; }
    int fourierLength() const { return cfg_->fourier_length; }
    int windowLength() const { return cfg_->window_length; }
    int windowOverlap() const { return cfg_->window_overlap; }
    std::pair<double, double> freqRange() const { return {cfg_->freq_lo, cfg_->freq_hi}; }
    int timeRange() const { return cfg_->time_range; }
    int spectrogramScaling() const { return cfg_->scaling; }
    std::vector<double> thresholds() const { return std::vector<double>(cfg_->thresholds, cfg_->thresholds + cfg_->n_thresholds); }
    int netInputs() const { return cfg_->layers[0].inputs; }
    int netOutputs() const { return cfg_->layers[cfg_->n_layers - 1].outputs; }
    const syldet_config_t *raw() const { return cfg_; }
    syldet_config_t *raw() { return cfg_; }

private:
    syldet_config_t *cfg_ = nullptr;
};

// A bank of independent detectors on one GPU (Processor.swift:57-59 keeps one SyllableDetector
// per channel; here they share one engine so that a batch of channels is one kernel launch).
class SyllableDetectorBank {
public:
    SyllableDetectorBank(const SyllableDetectorConfig &config, int channels, int device = 0, int engine = SYLDET_ENGINE_AUTO)
    {
        check(syldet_create(config.raw(), channels, device, engine, &h_));
        check(syldet_get_geometry(h_, &geometry_));
    }
    // a network per channel (ProcessorBase.init, Processor.swift:50-86): channel c runs configs[channelNet[c]]; the
    // configurations must be compatible (syldet_config_compatible)
    SyllableDetectorBank(const std::vector<const SyllableDetectorConfig *> &configs, const std::vector<int32_t> &channelNet, int device = 0,
                         int engine = SYLDET_ENGINE_AUTO)
    {
        std::vector<const syldet_config_t *> raw;
        for (const SyllableDetectorConfig *c : configs) raw.push_back(c ? c->raw() : nullptr);
        check(syldet_create_multi(raw.data(), (int32_t)raw.size(), channelNet.data(), (int32_t)channelNet.size(), device, engine, &h_));
        check(syldet_get_geometry(h_, &geometry_));
    }
    // networks that need only share the evaluation clock (syldet_create_mixed; ProcessorBase's rows each load their own file,
    // ViewControllerProcessor.swift:222-276): channel c runs configs[channelNet[c]], whatever its band, FFT size, chain or widths
    struct Mixed {};
    SyllableDetectorBank(Mixed, const std::vector<const SyllableDetectorConfig *> &configs, const std::vector<int32_t> &channelNet,
                         int device = 0, int engine = SYLDET_ENGINE_AUTO)
    {
        std::vector<const syldet_config_t *> raw;
        for (const SyllableDetectorConfig *c : configs) raw.push_back(c ? c->raw() : nullptr);
        check(syldet_create_mixed(raw.data(), (int32_t)raw.size(), channelNet.data(), (int32_t)channelNet.size(), device, engine, &h_));
        check(syldet_get_geometry(h_, &geometry_));
    }
    // channel c's own network's geometry (its class's bins, inputs and engine on a mixed bank)
    syldet_geometry_t channelGeometry(int32_t channel) const
    {
        syldet_geometry_t g;
        check(syldet_channel_geometry(h_, channel, &g));
        return g;
    }
    ~SyllableDetectorBank() { syldet_destroy(h_); }
    SyllableDetectorBank(const SyllableDetectorBank &) = delete;
    SyllableDetectorBank &operator=(const SyllableDetectorBank &) = delete;

    const syldet_geometry_t &geometry() const { return geometry_; }
    int channels() const { return syldet_channels(h_); }
    int64_t countEvaluations(int64_t samples) const { return syldet_count_evals(h_, samples); }

    // whole recordings, host buffers: samples [channels][n], outputs [channels][E][outputs], flags [channels][E]
    void run(const float *samples, int64_t n, std::vector<float> &outputs, std::vector<uint8_t> &flags)
    {
        const int64_t E = countEvaluations(n);
        outputs.assign((size_t)channels() * (size_t)E * (size_t)geometry_.outputs, 0.0f);
        flags.assign((size_t)channels() * (size_t)E, 0);
        check(syldet_run(h_, samples, n, n, outputs.data(), flags.data()));
    }
    // device buffers, asynchronous on `hipStream`
    void runDevice(const float *d_samples, int64_t n, int64_t stride, float *d_outputs, uint8_t *d_flags, void *hipStream)
    {
        check(syldet_run_device(h_, d_samples, n, stride, d_outputs, d_flags, hipStream));
    }
    // 16-bit PCM (sample x = x / 32768): the same calls, bit for bit their results on float(x) * 2^-15, half the bytes in
    void runPCM16(const int16_t *samples, int64_t n, std::vector<float> &outputs, std::vector<uint8_t> &flags)
    {
        const int64_t E = countEvaluations(n);
        outputs.assign((size_t)channels() * (size_t)E * (size_t)geometry_.outputs, 0.0f);
        flags.assign((size_t)channels() * (size_t)E, 0);
        check(syldet_run_s16(h_, samples, n, n, outputs.data(), flags.data()));
    }
    void runDevicePCM16(const int16_t *d_samples, int64_t n, int64_t stride, float *d_outputs, uint8_t *d_flags, void *hipStream)
    {
        check(syldet_run_device_s16(h_, d_samples, n, stride, d_outputs, d_flags, hipStream));
    }
    // interleaved 16-bit PCM frames [frames][channels]
    void runInterleavedPCM16(const int16_t *frames, int64_t n, std::vector<float> &outputs, std::vector<uint8_t> &flags)
    {
        const int64_t E = countEvaluations(n);
        outputs.assign((size_t)channels() * (size_t)(E > 0 ? E : 0) * (size_t)geometry_.outputs, 0.0f);
        flags.assign((size_t)channels() * (size_t)(E > 0 ? E : 0), 0);
        check(syldet_run_interleaved_s16(h_, frames, n, channels(), outputs.data(), flags.data()));
    }
    void runInterleavedDevicePCM16(const int16_t *d_frames, int64_t n, float *d_outputs, uint8_t *d_flags, void *hipStream)
    {
        check(syldet_run_interleaved_device_s16(h_, d_frames, n, channels(), d_outputs, d_flags, hipStream));
    }
    // live use: everything every channel has pending in one device round trip (the consumer loop of
    // Processor.swift:128-141 over all detectors); the detectors' processNewValue() then hand the results out
    int64_t processAll()
    {
        int64_t queued = 0;
        check(syldet_process_all(h_, &queued));
        return queued;
    }
    void appendInterleavedData(const float *data, int64_t frames) { check(syldet_append_interleaved(h_, data, frames, channels())); }
    void appendInterleavedDataPCM16(const int16_t *data, int64_t frames) { check(syldet_append_interleaved_s16(h_, data, frames, channels())); }
    // fromChannel / ofTotalChannels (CircularShortTimeFourierTransform.swift:203-217): the bank on a subset of a wider stream
    void appendInterleavedData(const float *data, int64_t frames, int32_t totalChannels, const int32_t *fromChannels)
    {
        check(syldet_append_interleaved_channels(h_, data, frames, totalChannels, fromChannels));
    }
    // TrackDetector's sample numbering and debounce (TrackDetector.swift:39-43, :65-100)
    std::vector<int64_t> detections(const uint8_t *flags, int64_t nEvals, double debounceSeconds, int channel)
    {
        std::vector<int64_t> idx((size_t)channels() * (size_t)nEvals), counts((size_t)channels());
        check(syldet_detections(h_, flags, nEvals, debounceSeconds, idx.data(), nEvals, counts.data()));
        return std::vector<int64_t>(idx.begin() + (size_t)channel * (size_t)nEvals,
                                    idx.begin() + (size_t)channel * (size_t)nEvals + (size_t)counts[(size_t)channel]);
    }
    // The Simulator's output track (ViewControllerSimulator.swift:251-344): output `output` of every channel as a fraction of
    // its threshold, held from one evaluation to the next, one value per sample: trace [channels][n] from outputs
    // [channels][nEvals][outputs] (host buffers, blocking)
    std::vector<float> trace(const float *outputs, int64_t nEvals, int64_t n, int32_t output = 0)
    {
        std::vector<float> t((size_t)channels() * (size_t)n);
        check(syldet_trace(h_, outputs, nEvals, output, t.data(), n, n));
        return t;
    }
    // device buffers, asynchronous on `hipStream`: fp32 rows, 16-bit rows (rint(v * 32767)), 16-bit frames [n][channels]
    void traceDevice(const float *d_outputs, int64_t nEvals, int32_t output, float *d_trace, int64_t n, int64_t stride, void *hipStream)
    {
        check(syldet_trace_device(h_, d_outputs, nEvals, output, d_trace, n, stride, hipStream));
    }
    void traceDevicePCM16(const float *d_outputs, int64_t nEvals, int32_t output, int16_t *d_trace, int64_t n, int64_t stride, void *hipStream)
    {
        check(syldet_trace_device_s16(h_, d_outputs, nEvals, output, d_trace, n, stride, hipStream));
    }
    void traceInterleavedDevicePCM16(const float *d_outputs, int64_t nEvals, int32_t output, int16_t *d_frames, int64_t n, void *hipStream)
    {
        check(syldet_trace_interleaved_device_s16(h_, d_outputs, nEvals, output, d_frames, n, hipStream));
    }
    // The TTL trigger track (Processor.swift:128-148, AudioInterface.swift:13-40, :442-445): the pulses the rig would have emitted for
    // flags [channels][nEvals] -- high for `width` samples from the render buffer behind every callback buffer of bufferLength
    // samples that made a flagged evaluation available, `latency` samples later.  track [channels][n] (host buffers, blocking)
    static int64_t triggerWidth(double seconds, double rate) { return syldet_trigger_width(seconds, rate); }
    std::vector<float> triggerTrack(const uint8_t *flags, int64_t nEvals, int64_t n, int64_t width, int32_t bufferLength = 32, int64_t latency = 0)
    {
        std::vector<float> t((size_t)channels() * (size_t)n);
        check(syldet_trigger(h_, flags, nEvals, bufferLength, width, latency, t.data(), n, n));
        return t;
    }
    std::vector<int16_t> triggerTrackPCM16(const uint8_t *flags, int64_t nEvals, int64_t n, int64_t width, int32_t bufferLength = 32,
                                           int64_t latency = 0)
    {
        std::vector<int16_t> t((size_t)channels() * (size_t)n);
        check(syldet_trigger_s16(h_, flags, nEvals, bufferLength, width, latency, t.data(), n, n));
        return t;
    }
    // the rising edges of one channel's track, as sample numbers
    std::vector<int64_t> triggerOnsets(const uint8_t *flags, int64_t nEvals, int64_t n, int64_t width, int32_t channel, int32_t bufferLength = 32,
                                       int64_t latency = 0)
    {
        const int64_t cap = std::min<int64_t>(nEvals, n / bufferLength + 1);
        std::vector<int64_t> idx((size_t)channels() * (size_t)std::max<int64_t>(cap, 1)), counts((size_t)channels());
        check(syldet_trigger_onsets(h_, flags, nEvals, bufferLength, width, latency, n, idx.data(), cap, counts.data()));
        return std::vector<int64_t>(idx.begin() + (size_t)channel * (size_t)cap,
                                    idx.begin() + (size_t)channel * (size_t)cap + (size_t)std::min(counts[(size_t)channel], cap));
    }
    // device buffers, asynchronous on `hipStream`: fp32 rows, 16-bit rows (32767 / 0), 16-bit frames [n][channels], 16-bit frames
    // [n][2 channels] with the recording's int16 rows beside the triggers, and the onsets
    void triggerDevice(const uint8_t *d_flags, int64_t nEvals, int32_t bufferLength, int64_t width, int64_t latency, float *d_track, int64_t n,
                       int64_t stride, void *hipStream)
    {
        check(syldet_trigger_device(h_, d_flags, nEvals, bufferLength, width, latency, d_track, n, stride, hipStream));
    }
    void triggerDevicePCM16(const uint8_t *d_flags, int64_t nEvals, int32_t bufferLength, int64_t width, int64_t latency, int16_t *d_track,
                            int64_t n, int64_t stride, void *hipStream)
    {
        check(syldet_trigger_device_s16(h_, d_flags, nEvals, bufferLength, width, latency, d_track, n, stride, hipStream));
    }
    void triggerInterleavedDevicePCM16(const uint8_t *d_flags, int64_t nEvals, int32_t bufferLength, int64_t width, int64_t latency,
                                       int16_t *d_frames, int64_t n, void *hipStream)
    {
        check(syldet_trigger_interleaved_device_s16(h_, d_flags, nEvals, bufferLength, width, latency, d_frames, n, hipStream));
    }
    void triggerMuxDevicePCM16(const uint8_t *d_flags, int64_t nEvals, int32_t bufferLength, int64_t width, int64_t latency,
                               const int16_t *d_samples, int64_t channelStride, int16_t *d_frames, int64_t n, void *hipStream)
    {
        check(syldet_trigger_mux_device_s16(h_, d_flags, nEvals, bufferLength, width, latency, d_samples, channelStride, d_frames, n, hipStream));
    }
    void triggerOnsetsDevice(const uint8_t *d_flags, int64_t nEvals, int32_t bufferLength, int64_t width, int64_t latency, int64_t n,
                             int64_t *d_indices, int64_t capacity, int64_t *d_counts, void *hipStream)
    {
        check(syldet_trigger_onsets_device(h_, d_flags, nEvals, bufferLength, width, latency, n, d_indices, capacity, d_counts, hipStream));
    }
    // the planar track and the onsets from one scan of the flags
    void triggerRehearseDevice(const uint8_t *d_flags, int64_t nEvals, int32_t bufferLength, int64_t width, int64_t latency, float *d_track,
                               int64_t n, int64_t stride, int64_t *d_indices, int64_t capacity, int64_t *d_counts, void *hipStream)
    {
        check(syldet_trigger_rehearse_device(h_, d_flags, nEvals, bufferLength, width, latency, d_track, n, stride, d_indices, capacity, d_counts, hipStream));
    }
    void triggerRehearseDevicePCM16(const uint8_t *d_flags, int64_t nEvals, int32_t bufferLength, int64_t width, int64_t latency, int16_t *d_track,
                                    int64_t n, int64_t stride, int64_t *d_indices, int64_t capacity, int64_t *d_counts, void *hipStream)
    {
        check(syldet_trigger_rehearse_device_s16(h_, d_flags, nEvals, bufferLength, width, latency, d_track, n, stride, d_indices, capacity, d_counts, hipStream));
    }
    // streaming: createHighOutput and renderOutput (AudioInterface.swift:442-445, :13-40) of one channel
    void armTrigger(int32_t channel, int64_t width) { check(syldet_trigger_arm(h_, channel, width)); }
    void renderTrigger(int32_t channel, float *out, int32_t nFrames) { check(syldet_trigger_render(h_, channel, out, nFrames)); }
    // The level meters of the rows (Processor.swift:111-113, :138, :158-184).  Whole recordings, host buffers, blocking: the RMS
    // readings [channels][M] of samples [channels][n] (M = levelsCount: one reading per buffersPerReading buffers of bufferLength
    // samples), and the output readings [channels][M] of outputs [channels][nEvals][outputs]
    static int64_t levelsCount(int64_t n, int32_t bufferLength, int64_t buffersPerReading)
    {
        return syldet_levels_count(n, bufferLength, buffersPerReading);
    }
    std::vector<double> levels(const float *samples, int64_t n, int32_t bufferLength, int64_t buffersPerReading)
    {
        std::vector<double> rms((size_t)channels() * (size_t)std::max<int64_t>(0, levelsCount(n, bufferLength, buffersPerReading)));
        check(syldet_levels(h_, samples, n, n, bufferLength, buffersPerReading, rms.data()));
        return rms;
    }
    std::vector<double> levelsPCM16(const int16_t *samples, int64_t n, int32_t bufferLength, int64_t buffersPerReading)
    {
        std::vector<double> rms((size_t)channels() * (size_t)std::max<int64_t>(0, levelsCount(n, bufferLength, buffersPerReading)));
        check(syldet_levels_s16(h_, samples, n, n, bufferLength, buffersPerReading, rms.data()));
        return rms;
    }
    std::vector<float> outputLevels(const float *outputs, int64_t nEvals, int64_t n, int32_t bufferLength, int64_t buffersPerReading,
                                    int32_t output = 0)
    {
        std::vector<float> lv((size_t)channels() * (size_t)std::max<int64_t>(0, levelsCount(n, bufferLength, buffersPerReading)));
        check(syldet_output_levels(h_, outputs, nEvals, output, n, bufferLength, buffersPerReading, lv.data()));
        return lv;
    }
    // device buffers, asynchronous on `hipStream`: the fp64 MEAN SQUARES [channels][M] (the RMS is their sqrt), fp32 output readings
    void levelsDevice(const float *d_samples, int64_t n, int64_t stride, int32_t bufferLength, int64_t buffersPerReading,
                      double *d_meanSquare, void *hipStream)
    {
        check(syldet_levels_device(h_, d_samples, n, stride, bufferLength, buffersPerReading, d_meanSquare, hipStream));
    }
    void levelsDevicePCM16(const int16_t *d_samples, int64_t n, int64_t stride, int32_t bufferLength, int64_t buffersPerReading,
                           double *d_meanSquare, void *hipStream)
    {
        check(syldet_levels_device_s16(h_, d_samples, n, stride, bufferLength, buffersPerReading, d_meanSquare, hipStream));
    }
    void levelsInterleavedDevice(const float *d_frames, int64_t n, int32_t bufferLength, int64_t buffersPerReading, double *d_meanSquare,
                                 void *hipStream)
    {
        check(syldet_levels_interleaved_device(h_, d_frames, n, channels(), bufferLength, buffersPerReading, d_meanSquare, hipStream));
    }
    void levelsInterleavedDevicePCM16(const int16_t *d_frames, int64_t n, int32_t bufferLength, int64_t buffersPerReading,
                                      double *d_meanSquare, void *hipStream)
    {
        check(syldet_levels_interleaved_device_s16(h_, d_frames, n, channels(), bufferLength, buffersPerReading, d_meanSquare, hipStream));
    }
    void outputLevelsDevice(const float *d_outputs, int64_t nEvals, int32_t output, int64_t n, int32_t bufferLength,
                            int64_t buffersPerReading, float *d_levels, void *hipStream)
    {
        check(syldet_output_levels_device(h_, d_outputs, nEvals, output, n, bufferLength, buffersPerReading, d_levels, hipStream));
    }
    // live use: getInputForChannel / getOutputForChannel (Processor.swift:158-184), read and reset, nullopt for no value; off
    // until enableMeters()
    void enableMeters(bool enable = true) { check(syldet_meters_enable(h_, enable ? 1 : 0)); }
    std::optional<double> getInputForChannel(int32_t channel)
    {
        double v = 0.0;
        int32_t has = 0;
        check(syldet_input_level(h_, channel, &v, &has));
        return has ? std::optional<double>(v) : std::nullopt;
    }
    std::optional<double> getOutputForChannel(int32_t channel)
    {
        double v = 0.0;
        int32_t has = 0;
        check(syldet_output_level(h_, channel, &v, &has));
        return has ? std::optional<double>(v) : std::nullopt;
    }
    syldet_t *raw() { return h_; }

private:
    syldet_t *h_ = nullptr;
    syldet_geometry_t geometry_{};
};

// One bank over several GPUs of this host, ONE process -- the reference's shape: ProcessorBase.init builds one detector per
// channel and one serial queue drains them all (Processor.swift:57-59,82,128-141; main.swift:86-89,126-130).  The library places
// a sub-bank and a stream on every listed device, splits the channels into contiguous blocks (time-axis ranges with a halo
// when there are fewer channels than devices) and gathers the flags with one RCCL all-gather of their bits per batch.
class SyllableDetectorShardedBank {
public:
    SyllableDetectorShardedBank(const SyllableDetectorConfig &config, int channels, const std::vector<int32_t> &devices,
                                int engine = SYLDET_ENGINE_AUTO, int exchange = SYLDET_EXCHANGE_RCCL)
    {
        check(syldet_create_sharded(config.raw(), channels, devices.data(), (int32_t)devices.size(), engine, exchange, &b_));
        try {
            check(syldet_get_geometry(syldet_sharded_bank(b_, 0), &geometry_));
        } catch (...) {                                            // (no destructor runs for a constructor that throws)
            syldet_sharded_destroy(b_);
            b_ = nullptr;
            throw;
        }
    }
    ~SyllableDetectorShardedBank() { syldet_sharded_destroy(b_); }
    SyllableDetectorShardedBank(const SyllableDetectorShardedBank &) = delete;
    SyllableDetectorShardedBank &operator=(const SyllableDetectorShardedBank &) = delete;

    const syldet_geometry_t &geometry() const { return geometry_; }
    int channels() const { return syldet_sharded_channels(b_); }
    int shards() const { return syldet_sharded_shards(b_); }
    int rcclRanks() const { return syldet_sharded_rccl_ranks(b_); }
    int launcherThreads() const { return syldet_sharded_launcher_threads(b_); }
    // brings the exchange up now (RCCL communicators, or peer access for the copy exchange); throws where the first gathering
    // batch would otherwise have -- a caller that wants to fall back makes the bank again with SYLDET_EXCHANGE_PEER_COPY
    void connect() { check(syldet_sharded_connect(b_)); }
    syldet_shard_t shard(int i) const
    {
        syldet_shard_t s;
        check(syldet_sharded_shard(b_, i, &s));
        return s;
    }
    int64_t countEvaluations(int64_t samples) const { return syldet_count_evals(syldet_sharded_bank(b_, 0), samples); }
    // whole recordings, host buffers: samples [channels][n] -> outputs [channels][E][outputs], flags [channels][E];
    // every device's copies and kernels are in flight together
    void run(const float *samples, int64_t n, std::vector<float> &outputs, std::vector<uint8_t> &flags)
    {
        const int64_t E = countEvaluations(n) > 0 ? countEvaluations(n) : 0;
        outputs.assign((size_t)channels() * (size_t)E * (size_t)geometry_.outputs, 0.0f);
        flags.assign((size_t)channels() * (size_t)E, 0);
        check(syldet_sharded_run(b_, samples, n, n, outputs.data(), flags.data()));
    }
    // per-shard device blocks (syldet_sharded_ranges says which samples shard i reads); flagsAll[i]: every channel's flags on
    // device i through the one exchange.  Asynchronous: synchronize() before reading.
    void runDevice(const float *const *d_samples, int64_t n, const int64_t *strides, float *const *d_outputs, uint8_t *const *d_flags,
                   uint8_t *const *d_flagsAll)
    {
        check(syldet_sharded_run_device(b_, d_samples, n, strides, d_outputs, d_flags, d_flagsAll));
    }
    void synchronize() { check(syldet_sharded_synchronize(b_)); }
    syldet_sharded_t *raw() { return b_; }

private:
    syldet_sharded_t *b_ = nullptr;
    syldet_geometry_t geometry_{};
};

// One channel of a bank with the reference's per-detector surface.
class SyllableDetector {
public:
    SyllableDetector(SyllableDetectorBank &bank, int channel) : bank_(bank), channel_(channel) {}

    void appendAudioData(const float *data, int64_t withSamples) { check(syldet_append(bank_.raw(), channel_, data, withSamples)); }
    void appendAudioDataPCM16(const int16_t *data, int64_t withSamples) { check(syldet_append_s16(bank_.raw(), channel_, data, withSamples)); }
    bool processNewValue() { const int r = syldet_process_new_value(bank_.raw(), channel_); check(r); return r == 1; }
    std::vector<float> lastOutputs() const
    {
        std::vector<float> out((size_t)bank_.geometry().outputs);
        check(syldet_last_outputs(bank_.raw(), channel_, out.data()));
        return out;
    }
    bool lastDetected() const { const int r = syldet_last_detected(bank_.raw(), channel_); check(r); return r == 1; }
    bool seenSyllable() { const int r = syldet_seen_syllable(bank_.raw(), channel_); check(r); return r == 1; }

private:
    SyllableDetectorBank &bank_;
    int channel_;
};

// ResamplerLinear (Resampler.swift:20-76) for `channels` streams fed in lock-step; state carries over between calls.
class ResamplerLinear {
public:
    ResamplerLinear(double fromRate, double toRate, int channels = 1, int device = 0) : channels_(channels)
    {
        check(syldet_resampler_create(fromRate, toRate, channels, device, &r_));
    }
    ~ResamplerLinear() { syldet_resampler_destroy(r_); }
    ResamplerLinear(const ResamplerLinear &) = delete;
    ResamplerLinear &operator=(const ResamplerLinear &) = delete;

    // host rows [channels][n] -> [channels][returned length]   (resampleArray, :71-75)
    std::vector<float> resampleArray(const std::vector<float> &arr)
    {
        const int64_t n = (int64_t)(arr.size() / (size_t)channels_), m = syldet_resampler_count(r_, n);
        std::vector<float> out((size_t)channels_ * (size_t)(m > 0 ? m : 0));
        int64_t got = 0;
        check(syldet_resample(r_, arr.data(), n, n, out.data(), m > 0 ? m : 1, &got));
        return out;
    }
    // device rows, asynchronous on `hipStream`   (resampleVector, :36-69)
    int64_t resampleVector(const float *d_data, int64_t n, int64_t stride, float *d_out, int64_t out_stride, void *hipStream)
    {
        int64_t got = 0;
        check(syldet_resample_device(r_, d_data, n, stride, d_out, out_stride, &got, hipStream));
        return got;
    }
    int64_t countOutput(int64_t n) const { return syldet_resampler_count(r_, n); }

private:
    syldet_resampler_t *r_ = nullptr;
    int channels_;
};

// ResamplerSinc: the band-limited converter (syldet_convert_rate_sinc_device's convention) as a second conformer of the
// reference's Resampler protocol (Resampler.swift:12-15), for `channels` streams fed in lock-step.  Push blocks of any sizes,
// then flush: the concatenated outputs are the whole-recording call's, bit for bit.  Quality arguments below zero take
// syldet_sinc_defaults'.  All device work of one object belongs on one stream.
class ResamplerSinc {
public:
    ResamplerSinc(double fromRate, double toRate, int channels = 1, int device = 0, int zeroCrossings = -1, double beta = -1.0,
                  double rolloff = -1.0) : channels_(channels)
    {
        int32_t z = 0;
        double b = 0.0, r = 0.0;
        syldet_sinc_defaults(&z, &b, &r);
        check(syldet_sinc_resampler_create(fromRate, toRate, channels, device, zeroCrossings < 0 ? z : zeroCrossings, beta < 0.0 ? b : beta,
                                           rolloff < 0.0 ? r : rolloff, &r_));
    }
    ~ResamplerSinc() { syldet_sinc_resampler_destroy(r_); }
    ResamplerSinc(const ResamplerSinc &) = delete;
    ResamplerSinc &operator=(const ResamplerSinc &) = delete;

    // host rows [channels][n] -> [channels][returned length], blocking
    std::vector<float> resampleArray(const std::vector<float> &arr)
    {
        const int64_t n = (int64_t)(arr.size() / (size_t)channels_), m = syldet_sinc_resampler_count(r_, n);
        std::vector<float> out((size_t)channels_ * (size_t)m);
        int64_t got = 0;
        check(syldet_sinc_resample(r_, arr.data(), n, n, out.data(), m > 0 ? m : 1, &got));
        return out;
    }
    // the recording's last outputs, host rows [channels][returned length]; the stream is finished until reset()
    std::vector<float> flush()
    {
        const int64_t m = syldet_sinc_resampler_flush_count(r_);
        std::vector<float> out((size_t)channels_ * (size_t)m);
        int64_t got = 0;
        check(syldet_sinc_resampler_flush(r_, out.data(), m > 0 ? m : 1, &got));
        return out;
    }
    // device rows, asynchronous on `hipStream`
    int64_t resampleVector(const float *d_data, int64_t n, int64_t stride, float *d_out, int64_t out_stride, void *hipStream)
    {
        int64_t got = 0;
        check(syldet_sinc_resample_device(r_, d_data, n, stride, d_out, out_stride, &got, hipStream));
        return got;
    }
    int64_t resampleVectorPCM16(const int16_t *d_data, int64_t n, int64_t stride, float *d_out, int64_t out_stride, void *hipStream)
    {
        int64_t got = 0;
        check(syldet_sinc_resample_device_s16(r_, d_data, n, stride, d_out, out_stride, &got, hipStream));
        return got;
    }
    int64_t flushDevice(float *d_out, int64_t out_stride, void *hipStream)
    {
        int64_t got = 0;
        check(syldet_sinc_resampler_flush_device(r_, d_out, out_stride, &got, hipStream));
        return got;
    }
    void reset() { check(syldet_sinc_resampler_reset(r_)); }
    int64_t countOutput(int64_t n) const { return syldet_sinc_resampler_count(r_, n); }
    int64_t countFlush() const { return syldet_sinc_resampler_flush_count(r_); }
    int64_t samplesIn() const { int64_t n = 0; check(syldet_sinc_resampler_position(r_, &n, nullptr, nullptr)); return n; }
    int64_t samplesOut() const { int64_t m = 0; check(syldet_sinc_resampler_position(r_, nullptr, &m, nullptr)); return m; }
    bool finished() const { int32_t f = 0; check(syldet_sinc_resampler_position(r_, nullptr, nullptr, &f)); return f != 0; }

private:
    syldet_sinc_resampler_t *r_ = nullptr;
    int channels_;
};

}  // namespace syldetxx
