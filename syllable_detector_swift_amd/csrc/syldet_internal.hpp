// syldet_internal.hpp -- shared declarations of libsyldet's host side (not installed).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "syldet.h"

namespace sd {

// Thread-local text of the last failing call (syldet_last_error).
void set_error(const std::string &msg);
int fail(int status, const std::string &msg);

// A HIP call that must succeed: the call's text and the runtime's message become the last error, the status SYLDET_ERR_DEVICE
// (for the files that include the HIP runtime's header).
#define SYLDET_HIP(expr)                                                                         \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return fail(SYLDET_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));  \
    } while (0)

// Deep, self-owned copy of a syldet_config_t.  `view` points into the vectors.
struct OwnedConfig {
    syldet_config_t view{};
    std::vector<syldet_fn_t> input_fns, output_fns;
    std::vector<syldet_layer_t> layers;
    std::vector<std::vector<float>> fn_xoff_in, fn_gain_in, fn_xoff_out, fn_gain_out;
    std::vector<std::vector<float>> weights, biases;
    std::vector<double> thresholds;

    OwnedConfig() = default;
    OwnedConfig(const OwnedConfig &) = delete;
    OwnedConfig &operator=(const OwnedConfig &) = delete;

    int assign(const syldet_config_t &src);   // validates pointers, copies arrays
    void relink();                             // re-point view at the vectors
};

// SyllableDetector.init's validation (SyllableDetector.swift:42-60) plus the STFT
// constructor's (CircularShortTimeFourierTransform.swift:61-96).
int compute_geometry(const syldet_config_t &cfg, syldet_geometry_t *out);

void make_window(int window, int length, float *out);

// The library's sum of squares (syldet_levels.cpp, include/syldet.h): n samples `step` elements apart; int16 x is float(x) * 2^-15.
float sum_squares_tree(const float *x, int64_t n, int64_t step);
float sum_squares_tree(const int16_t *x, int64_t n, int64_t step);
// is L a buffer length the level meters take (a power of two in [8, 4096])?
inline bool levels_buffer_ok(int64_t L) { return L >= 8 && L <= 4096 && (L & (L - 1)) == 0; }
// ... and the refusal of one that is not, for every call that takes a buffer length (the meters, the trigger, the packed recordings' too)
inline int buffer_length_arg(int64_t L)
{
    return levels_buffer_ok(L) ? SYLDET_OK : fail(SYLDET_ERR_INVALID_ARGUMENT, "buffer_length must be a power of two in [8, 4096]");
}

// syldet_count_frames and syldet_count_evals from the clock alone: a handle's, or a configuration's (syldet_recordings_plan_of_config)
inline int64_t count_frames(const syldet_geometry_t &g, int window_length, int64_t S)
{
    const int64_t need = (int64_t)g.gap + window_length;    // :286-288
    return S < need ? 0 : (S - need) / g.hop + 1;            // consume hop per frame :299-302
}
inline int64_t count_evals(const syldet_geometry_t &g, int window_length, int time_range, int64_t S)
{
    const int64_t J = count_frames(g, window_length, S);
    return J >= time_range ? J - time_range + 1 : 0;         // SyllableDetector.swift:164-178
}

// What the packed recordings' plan and the scorer need of a bank -- a handle's, or (syldet_recordings_plan_of_config) a configuration's without one: channel_net is the caller's table of
// syldet_create_multi / syldet_create_mixed ([channels], the handle's own memory), NULL on a plain bank.
struct BankInfo {
    int channels, device;
    double sampling_rate;
    int window_length, time_range;
    syldet_geometry_t geom;
    const int *channel_net;
};
void bank_info(const syldet_t *h, BankInfo *out);

// The band-limited converter's host side (syldet_resampler.cpp), for the packed recordings' converting load (syldet_recordings.cpp).
// sinc_quality: the ranges of Z, beta and rolloff (SYLDET_ERR_INVALID_ARGUMENT).  sinc_design: s and H of the sinc convention of
// include/syldet.h with the statuses of syldet_convert_rate_sinc_device in their order -- the rates, sinc_quality, the ratio, H.
int sinc_quality(int32_t Z, double beta, double rho);
int sinc_design(double rate_in, double rate_out, int32_t Z, double beta, double rho, double *s, double *H);
// Calls use(table, entries, ctx) with the unit filter's table of (Z, beta) on the current device (the cache of
// syldet_convert_rate_sinc_device: a blocking copy on first use), holding the cache's lock until use returns: use queues the
// launch that reads the table.  Returns use's status, or the lookup's.
int sinc_table_use(int32_t Z, double beta, int (*use)(const float *table, int entries, void *ctx), void *ctx);

}  // namespace sd
