// syldet_resampler.cpp -- ResamplerLinear (Common/Resampler.swift:20-76) for a bank of channels on the
// device, and the stand-alone de-interleave entry point.  The resampling state that depends only on
// sizes (`offset`) lives on the host and is advanced with the reference's own fp32 operations; the
// per-channel carry (`last`) lives on the device next to the data.  The two stateless whole-recording converters are here too:
// the linear one and the band-limited one (a Kaiser-windowed sinc: its design, its fp64 coefficient and its table cache) -- and
// the band-limited one's streaming form, ResamplerSinc: the same outputs block by block (sinc_stream.hpp holds its arithmetic).

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "sinc_stream.hpp"
#include "syldet_internal.hpp"

using namespace sd;

struct syldet_resampler {
    double rate_in = 0, rate_out = 0;
    int channels = 0, device = 0;
    float step = 1.0f;               // Float(samplingRateIn / samplingRateOut), :33
    float offset = 0.0f;             // :26
    float *d_last = nullptr;         // [channels], :25
    float *d_in = nullptr, *d_out = nullptr;   // staging of the host-pointer entry point
    size_t in_cap = 0, out_cap = 0;
    hipStream_t stream = nullptr;
};

extern "C" {

int syldet_resampler_create(double rate_in, double rate_out, int32_t n_channels, int32_t device, syldet_resampler_t **out)
{
    if (!out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (!(rate_in > 0.0) || !(rate_out > 0.0)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "sampling rates must be positive");
    if (n_channels <= 0 || n_channels > 65535) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_channels must be in [1, 65535]");
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0)
        return fail(SYLDET_ERR_NO_DEVICE, std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count is 0"));
    if (device < 0 || device >= n_dev) return fail(SYLDET_ERR_NO_DEVICE, "device index out of range");
    std::unique_ptr<syldet_resampler> r(new (std::nothrow) syldet_resampler());
    if (!r) return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    r->rate_in = rate_in; r->rate_out = rate_out; r->channels = n_channels; r->device = device;
    r->step = (float)(rate_in / rate_out);
    // device resources; on any failure the partially built handle is torn down like a finished one
    auto bring_up = [&]() -> int {
        SYLDET_HIP(hipSetDevice(device));
        SYLDET_HIP(hipMalloc((void **)&r->d_last, (size_t)n_channels * sizeof(float)));
        SYLDET_HIP(hipMemset(r->d_last, 0, (size_t)n_channels * sizeof(float)));
        SYLDET_HIP(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
        return SYLDET_OK;
    };
    if (int st = bring_up()) {
        syldet_resampler_destroy(r.release());
        return st;
    }
    *out = r.release();
    return SYLDET_OK;
}

int syldet_resampler_destroy(syldet_resampler_t *r)
{
    if (!r) return SYLDET_OK;
    (void)hipSetDevice(r->device);
    if (r->stream) { (void)hipStreamSynchronize(r->stream); (void)hipStreamDestroy(r->stream); }
    if (r->d_last) (void)hipFree(r->d_last);
    if (r->d_in) (void)hipFree(r->d_in);
    if (r->d_out) (void)hipFree(r->d_out);
    delete r;
    return SYLDET_OK;
}

int64_t syldet_resampler_count(const syldet_resampler_t *r, int64_t n_in)
{
    if (!r || n_in <= 0) return 0;
    const int64_t n = (int64_t)(((float)n_in - r->offset) / r->step);    // Int((Float(numSamplesIn) - offset) / step), :40
    return n > 0 ? n : 0;
}

int syldet_resample_device(syldet_resampler_t *r, const float *d_in, int64_t n_in, int64_t in_stride, float *d_out,
                           int64_t out_stride, int64_t *n_out, void *hip_stream)
{
    if (!r) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (n_out) *n_out = 0;
    if (n_in < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_in must be >= 0");
    const int64_t n = syldet_resampler_count(r, n_in);
    if (n_in == 0 || n <= 0) return SYLDET_OK;        // nothing to emit; the reference would index an empty array here
    if (!d_in || !d_out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL buffer");
    if ((r->channels > 1 && in_stride < n_in) || (r->channels > 1 && out_stride < n))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "row strides must cover the rows");
    SYLDET_HIP(hipSetDevice(r->device));
    SYLDET_HIP(launch_resample_linear(d_in, n_in, in_stride, d_out, n, out_stride, r->channels, r->step, r->offset, r->d_last,
                                      (hipStream_t)hip_stream));
    // offset = indices[numSamplesOut - 1] + step - Float(numSamplesIn - 1), :65, with indices[0] = 0 after :54-56
    float last_index = r->offset + (float)(n - 1) * r->step;
    if (r->offset < 0.0f && n == 1) last_index = 0.0f;
    r->offset = last_index + r->step - (float)(n_in - 1);
    if (n_out) *n_out = n;
    return SYLDET_OK;
}

int syldet_resample(syldet_resampler_t *r, const float *in, int64_t n_in, int64_t in_stride, float *out, int64_t out_stride,
                    int64_t *n_out)
{
    if (!r) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (n_out) *n_out = 0;
    if (n_in < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_in must be >= 0");
    const int64_t n = syldet_resampler_count(r, n_in);
    if (n_in == 0 || n <= 0) return SYLDET_OK;
    if (!in || !out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL buffer");
    SYLDET_HIP(hipSetDevice(r->device));
    const size_t C = (size_t)r->channels, ib = C * (size_t)n_in * sizeof(float), ob = C * (size_t)n * sizeof(float);
    if (ib > r->in_cap) {
        if (r->d_in) (void)hipFree(r->d_in);
        r->d_in = nullptr; r->in_cap = 0;
        SYLDET_HIP(hipMalloc((void **)&r->d_in, ib));
        r->in_cap = ib;
    }
    if (ob > r->out_cap) {
        if (r->d_out) (void)hipFree(r->d_out);
        r->d_out = nullptr; r->out_cap = 0;
        SYLDET_HIP(hipMalloc((void **)&r->d_out, ob));
        r->out_cap = ob;
    }
    SYLDET_HIP(hipMemcpy2DAsync(r->d_in, (size_t)n_in * sizeof(float), in, (size_t)(C > 1 ? in_stride : n_in) * sizeof(float),
                                (size_t)n_in * sizeof(float), C, hipMemcpyHostToDevice, r->stream));
    if (int st = syldet_resample_device(r, r->d_in, n_in, n_in, r->d_out, n, n_out, r->stream)) return st;
    SYLDET_HIP(hipMemcpy2DAsync(out, (size_t)(C > 1 ? out_stride : n) * sizeof(float), r->d_out, (size_t)n * sizeof(float),
                                (size_t)n * sizeof(float), C, hipMemcpyDeviceToHost, r->stream));
    SYLDET_HIP(hipStreamSynchronize(r->stream));
    return SYLDET_OK;
}

int64_t syldet_convert_rate_count(int64_t n_in, double rate_in, double rate_out)
{
    if (n_in <= 0 || !(rate_in > 0.0) || !(rate_out > 0.0)) return 0;
    return (int64_t)((double)(n_in - 1) * rate_out / rate_in) + 1;       // positions i * rate_in / rate_out <= n_in - 1
}

int syldet_convert_rate_device(const float *d_in, int64_t n_in, int64_t in_stride, int32_t n_channels, double rate_in,
                               double rate_out, float *d_out, int64_t out_stride, int64_t *n_out, void *hip_stream)
{
    if (n_out) *n_out = 0;
    if (n_in < 0 || n_channels <= 0 || !(rate_in > 0.0) || !(rate_out > 0.0)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    const int64_t n = syldet_convert_rate_count(n_in, rate_in, rate_out);
    if (n <= 0) return SYLDET_OK;
    if (!d_in || !d_out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (n_channels > 1 && (in_stride < n_in || out_stride < n)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "row strides must cover the rows");
    SYLDET_HIP(launch_convert_rate(d_in, n_in, in_stride, d_out, n, out_stride, n_channels, rate_in / rate_out, (hipStream_t)hip_stream));
    if (n_out) *n_out = n;
    return SYLDET_OK;
}

}  // extern "C"

// ---- the band-limited converter (the sinc convention of include/syldet.h) ----
namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr double kSincMaxHalfWidth = 65536.0;          // H = Z / s: every output costs 2 H taps, so this bounds a launch's run time

// I0 by its power series, sum ((x / 2)^k / k!)^2: every term positive, so no cancellation; x <= 20 ends within 60 terms
double bessel_i0(double x)
{
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

double sinc_pi(double x)
{
    const double y = kPi * x;
    return y == 0.0 ? 1.0 : std::sin(y) / y;
}

}  // namespace

// the ranges of the quality (syldet_internal.hpp)
int sd::sinc_quality(int32_t Z, double beta, double rho)
{
    if (Z < 4 || Z > 64) return fail(SYLDET_ERR_INVALID_ARGUMENT, "zero_crossings must be in [4, 64]");
    if (!(beta >= 0.0 && beta <= 20.0)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "beta must be in [0, 20]");
    if (!(rho > 0.0 && rho <= 1.0)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "rolloff must be in (0, 1]");
    return SYLDET_OK;
}

// s and H of the convention; the statuses of the device calls, in their order (syldet_internal.hpp: the packed recordings'
// converting load designs every recording through this function too, so its scalars are these doubles)
int sd::sinc_design(double rate_in, double rate_out, int32_t Z, double beta, double rho, double *s, double *H)
{
    if (!(rate_in > 0.0) || !(rate_out > 0.0) || !std::isfinite(rate_in) || !std::isfinite(rate_out))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "sampling rates must be positive");
    if (int st = sinc_quality(Z, beta, rho)) return st;
    const double ratio = rate_in / rate_out;
    if (!(ratio >= 1.0 / 16.0 && ratio <= 16.0)) return fail(SYLDET_ERR_UNSUPPORTED, "rate_in / rate_out must be in [1/16, 16]");
    *s = (rate_out / rate_in < 1.0 ? rate_out / rate_in : 1.0) * rho;
    *H = (double)Z / *s;
    if (!(*H <= kSincMaxHalfWidth)) return fail(SYLDET_ERR_UNSUPPORTED, "the filter's half width Z / s exceeds 65536 input samples");
    return SYLDET_OK;
}

namespace {

// The unit filter's table on the host: g[j] = sinc(j Z / N) * kaiser(j / N) for j < N = sinc_table_entries(Z), zeros from g[N] on
// (N + 4 floats).  The one place its values are made: the cache below and every streaming handle copy these floats.
std::vector<float> sinc_table_values(int Z, double beta)
{
    const int N = sinc_table_entries(Z);
    std::vector<float> g((size_t)N + 4, 0.0f);
    const double i0b = bessel_i0(beta);
    for (int j = 0; j < N; j++) {
        const double u = (double)j / (double)N;
        g[(size_t)j] = (float)(sinc_pi(u * (double)Z) * bessel_i0(beta * std::sqrt(1.0 - u * u)) / i0b);
    }
    return g;
}

// The unit filter's table on the device, one per (device, Z, beta), made on the first call that needs it (a blocking copy) and
// kept for the life of the process; at most kSincTables of them, the oldest given up once a new one is in place.  The caller
// holds g_sinc_mutex from the lookup to the end of its launch: hipFree waits for the work already queued, so a table is never
// freed between a lookup and the launch that reads it.
struct SincTable { int device; int Z; double beta; float *d; };
constexpr size_t kSincTables = 16;
std::mutex g_sinc_mutex;
std::vector<SincTable> g_sinc_tables;

int sinc_table(int Z, double beta, const float **out, int *entries)
{
    int device = 0;
    SYLDET_HIP(hipGetDevice(&device));
    const int N = sinc_table_entries(Z);
    *entries = N;
    for (const SincTable &t : g_sinc_tables)
        if (t.device == device && t.Z == Z && t.beta == beta) { *out = t.d; return SYLDET_OK; }
    const std::vector<float> g = sinc_table_values(Z, beta);
    float *d = nullptr;
    SYLDET_HIP(hipMalloc((void **)&d, g.size() * sizeof(float)));
    hipError_t e = hipMemcpy(d, g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail(SYLDET_ERR_DEVICE, std::string("hipMemcpy of the filter table: ") + hipGetErrorString(e));
    }
    if (g_sinc_tables.size() >= kSincTables) {
        (void)hipFree(g_sinc_tables.front().d);
        g_sinc_tables.erase(g_sinc_tables.begin());
    }
    g_sinc_tables.push_back({device, Z, beta, d});
    *out = d;
    return SYLDET_OK;
}

template <typename T>
int convert_rate_sinc(const T *d_in, int64_t n_in, int64_t in_stride, int32_t n_channels, double rate_in, double rate_out,
                      int32_t Z, double beta, double rho, float *d_out, int64_t out_stride, int64_t *n_out, void *hip_stream)
{
    if (n_out) *n_out = 0;
    if (n_in < 0 || n_channels <= 0 || n_channels > 65535) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_in must be >= 0, n_channels in [1, 65535]");
    if (!d_in || !d_out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL buffer");
    double s = 0.0, H = 0.0;
    // (the ranges before the ratio: a bad parameter is an invalid argument at any ratio)
    if (int st = sinc_design(rate_in, rate_out, Z, beta, rho, &s, &H)) return st;
    const int64_t n = syldet_convert_rate_count(n_in, rate_in, rate_out);
    if (n_channels > 1 && (in_stride < n_in || out_stride < n)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "row strides must cover the rows");
    if (n <= 0) return SYLDET_OK;
    const float *table = nullptr;
    int N = 0;
    std::lock_guard<std::mutex> lock(g_sinc_mutex);          // from the table's lookup to the end of the launch (see sinc_table)
    if (int st = sinc_table(Z, beta, &table, &N)) return st;
    if constexpr (sizeof(T) == 2)
        SYLDET_HIP(launch_convert_rate_sinc_s16(d_in, n_in, in_stride, d_out, n, out_stride, n_channels, rate_in, rate_out, H, (float)s,
                                                table, N, (hipStream_t)hip_stream));
    else
        SYLDET_HIP(launch_convert_rate_sinc(d_in, n_in, in_stride, d_out, n, out_stride, n_channels, rate_in, rate_out, H, (float)s,
                                            table, N, (hipStream_t)hip_stream));
    if (n_out) *n_out = n;
    return SYLDET_OK;
}

}  // namespace

int sd::sinc_table_use(int32_t Z, double beta, int (*use)(const float *table, int entries, void *ctx), void *ctx)
{
    const float *table = nullptr;
    int N = 0;
    std::lock_guard<std::mutex> lock(g_sinc_mutex);          // from the table's lookup to the end of the launch (see sinc_table)
    if (int st = sinc_table(Z, beta, &table, &N)) return st;
    return use(table, N, ctx);
}

// ---- the streaming form (the streaming sinc convention of include/syldet.h) ----
struct syldet_sinc_resampler {
    double rate_in = 0, rate_out = 0, beta = 0, rho = 0, s = 0, H = 0;
    int Z = 0, channels = 0, device = 0;
    int64_t L = 0;                   // the history's capacity a channel: ceil(2 H) + 2
    int64_t n_in_total = 0;          // N
    int64_t n_out_total = 0;         // M = ready(N) until the flush
    bool finished = false;
    float *d_table = nullptr;        // the handle's own copy of the unit filter's table
    int entries = 0;
    float *d_hist[2] = {nullptr, nullptr};     // [channels][L] each: the kernels of a push read one and write the other
    int cur = 0;
    float *d_in = nullptr, *d_out = nullptr;   // staging of the host-pointer entry points
    size_t in_cap = 0, out_cap = 0;
    hipStream_t stream = nullptr;
};

namespace {

// The statuses of a push, in their order, and the number of outputs it emits; nothing is touched.
int sinc_push_check(const syldet_sinc_resampler *r, bool have_in, int64_t n_in, int64_t in_stride, bool have_out, int64_t out_stride,
                    int64_t *emit)
{
    *emit = 0;
    if (n_in < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_in must be >= 0");
    if (r->finished) return fail(SYLDET_ERR_INVALID_ARGUMENT, "the stream is finished (flushed): reset it before the next push");
    if (n_in == 0) return SYLDET_OK;
    if (n_in > ((int64_t)1 << 62) - r->n_in_total) return fail(SYLDET_ERR_INVALID_ARGUMENT, "more than 2^62 samples in one stream");
    if (!have_in) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL buffer");
    const int64_t n = sinc_stream_ready(r->n_in_total + n_in, r->rate_in, r->rate_out, r->H) - r->n_out_total;
    if (n > 0 && !have_out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (r->channels > 1 && (in_stride < n_in || (n > 0 && out_stride < n)))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "row strides must cover the rows");
    *emit = n;
    return SYLDET_OK;
}

int sinc_flush_check(const syldet_sinc_resampler *r, bool have_out, int64_t out_stride, int64_t *emit)
{
    *emit = 0;
    if (r->finished) return SYLDET_OK;                       // a second flush emits nothing
    const int64_t n = syldet_convert_rate_count(r->n_in_total, r->rate_in, r->rate_out) - r->n_out_total;
    if (n > 0 && !have_out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (r->channels > 1 && n > 0 && out_stride < n) return fail(SYLDET_ERR_INVALID_ARGUMENT, "row strides must cover the rows");
    *emit = n > 0 ? n : 0;
    return SYLDET_OK;
}

template <typename T>
int sinc_push_device(syldet_sinc_resampler *r, const T *d_in, int64_t n_in, int64_t in_stride, float *d_out, int64_t out_stride,
                     int64_t *n_out, void *hip_stream)
{
    if (!r) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (n_out) *n_out = 0;
    int64_t emit = 0;
    if (int st = sinc_push_check(r, d_in != nullptr, n_in, in_stride, d_out != nullptr, out_stride, &emit)) return st;
    if (n_in == 0) return SYLDET_OK;
    // host arithmetic is done; from here on only launches (no allocation, no copy, no wait)
    SYLDET_HIP(hipSetDevice(r->device));
    const float *hist = r->d_hist[r->cur];
    float *next = r->d_hist[r->cur ^ 1];
    if constexpr (sizeof(T) == 2)
        SYLDET_HIP(launch_sinc_stream_push_s16(hist, next, r->L, d_in, n_in, in_stride, r->n_in_total, d_out, out_stride, r->n_out_total,
                                               emit, r->channels, r->rate_in, r->rate_out, r->H, (float)r->s, r->d_table, r->entries,
                                               (hipStream_t)hip_stream));
    else
        SYLDET_HIP(launch_sinc_stream_push(hist, next, r->L, d_in, n_in, in_stride, r->n_in_total, d_out, out_stride, r->n_out_total,
                                           emit, r->channels, r->rate_in, r->rate_out, r->H, (float)r->s, r->d_table, r->entries,
                                           (hipStream_t)hip_stream));
    r->cur ^= 1;
    r->n_in_total += n_in;
    r->n_out_total += emit;
    if (n_out) *n_out = emit;
    return SYLDET_OK;
}

// the host-pointer entry points' staging rows: [channels][n] each, grown as needed
int sinc_stage(syldet_sinc_resampler *r, int64_t n_in, int64_t n_out)
{
    const size_t C = (size_t)r->channels, ib = C * (size_t)n_in * sizeof(float), ob = C * (size_t)n_out * sizeof(float);
    if (ib > r->in_cap) {
        if (r->d_in) (void)hipFree(r->d_in);
        r->d_in = nullptr; r->in_cap = 0;
        SYLDET_HIP(hipMalloc((void **)&r->d_in, ib));
        r->in_cap = ib;
    }
    if (ob > r->out_cap) {
        if (r->d_out) (void)hipFree(r->d_out);
        r->d_out = nullptr; r->out_cap = 0;
        SYLDET_HIP(hipMalloc((void **)&r->d_out, ob));
        r->out_cap = ob;
    }
    return SYLDET_OK;
}

}  // namespace

extern "C" {

int64_t syldet_sinc_ready(int64_t n_in_total, double rate_in, double rate_out, int32_t zero_crossings, double rolloff)
{
    double s = 0.0, H = 0.0;
    if (sinc_design(rate_in, rate_out, zero_crossings, 0.0, rolloff, &s, &H)) return -1;
    return sinc_stream_ready(n_in_total, rate_in, rate_out, H);
}

int syldet_sinc_resampler_create(double rate_in, double rate_out, int32_t n_channels, int32_t device, int32_t zero_crossings,
                                 double beta, double rolloff, syldet_sinc_resampler_t **out)
{
    if (!out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (n_channels <= 0 || n_channels > 65535) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_channels must be in [1, 65535]");
    double s = 0.0, H = 0.0;
    if (int st = sinc_design(rate_in, rate_out, zero_crossings, beta, rolloff, &s, &H)) return st;
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0)
        return fail(SYLDET_ERR_NO_DEVICE, std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count is 0"));
    if (device < 0 || device >= n_dev) return fail(SYLDET_ERR_NO_DEVICE, "device index out of range");
    std::unique_ptr<syldet_sinc_resampler> r(new (std::nothrow) syldet_sinc_resampler());
    if (!r) return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    r->rate_in = rate_in; r->rate_out = rate_out; r->beta = beta; r->rho = rolloff; r->s = s; r->H = H;
    r->Z = zero_crossings; r->channels = n_channels; r->device = device;
    r->L = sinc_stream_history(H);
    r->entries = sinc_table_entries(zero_crossings);
    auto bring_up = [&]() -> int {
        SYLDET_HIP(hipSetDevice(device));
        const std::vector<float> g = sinc_table_values(zero_crossings, beta);
        SYLDET_HIP(hipMalloc((void **)&r->d_table, g.size() * sizeof(float)));
        SYLDET_HIP(hipMemcpy(r->d_table, g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice));
        const size_t hb = (size_t)n_channels * (size_t)r->L * sizeof(float);
        for (int b = 0; b < 2; b++) {
            SYLDET_HIP(hipMalloc((void **)&r->d_hist[b], hb));
            SYLDET_HIP(hipMemset(r->d_hist[b], 0, hb));
        }
        SYLDET_HIP(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
        SYLDET_HIP(hipDeviceSynchronize());                  // the table and the zeros are in place before any stream reads them
        return SYLDET_OK;
    };
    if (int st = bring_up()) {
        syldet_sinc_resampler_destroy(r.release());
        return st;
    }
    *out = r.release();
    return SYLDET_OK;
}

int syldet_sinc_resampler_destroy(syldet_sinc_resampler_t *r)
{
    if (!r) return SYLDET_OK;
    (void)hipSetDevice(r->device);
    if (r->stream) { (void)hipStreamSynchronize(r->stream); (void)hipStreamDestroy(r->stream); }
    if (r->d_table) (void)hipFree(r->d_table);               // (hipFree waits for the work already queued)
    for (int b = 0; b < 2; b++)
        if (r->d_hist[b]) (void)hipFree(r->d_hist[b]);
    if (r->d_in) (void)hipFree(r->d_in);
    if (r->d_out) (void)hipFree(r->d_out);
    delete r;
    return SYLDET_OK;
}

int syldet_sinc_resampler_reset(syldet_sinc_resampler_t *r)
{
    if (!r) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    r->n_in_total = 0; r->n_out_total = 0; r->finished = false;      // (an empty history: nothing of the buffers is read)
    return SYLDET_OK;
}

int syldet_sinc_resampler_position(const syldet_sinc_resampler_t *r, int64_t *n_in_total, int64_t *n_out_total, int32_t *finished)
{
    if (!r) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (n_in_total) *n_in_total = r->n_in_total;
    if (n_out_total) *n_out_total = r->n_out_total;
    if (finished) *finished = r->finished ? 1 : 0;
    return SYLDET_OK;
}

int64_t syldet_sinc_resampler_count(const syldet_sinc_resampler_t *r, int64_t n_in)
{
    if (!r || n_in <= 0 || r->finished || n_in > ((int64_t)1 << 62) - r->n_in_total) return 0;
    return sinc_stream_ready(r->n_in_total + n_in, r->rate_in, r->rate_out, r->H) - r->n_out_total;
}

int64_t syldet_sinc_resampler_flush_count(const syldet_sinc_resampler_t *r)
{
    if (!r || r->finished) return 0;
    const int64_t n = syldet_convert_rate_count(r->n_in_total, r->rate_in, r->rate_out) - r->n_out_total;
    return n > 0 ? n : 0;
}

int syldet_sinc_resample_device(syldet_sinc_resampler_t *r, const float *d_in, int64_t n_in, int64_t in_stride, float *d_out,
                                int64_t out_stride, int64_t *n_out, void *hip_stream)
{
    return sinc_push_device<float>(r, d_in, n_in, in_stride, d_out, out_stride, n_out, hip_stream);
}

int syldet_sinc_resample_device_s16(syldet_sinc_resampler_t *r, const int16_t *d_in, int64_t n_in, int64_t in_stride, float *d_out,
                                    int64_t out_stride, int64_t *n_out, void *hip_stream)
{
    return sinc_push_device<int16_t>(r, d_in, n_in, in_stride, d_out, out_stride, n_out, hip_stream);
}

int syldet_sinc_resampler_flush_device(syldet_sinc_resampler_t *r, float *d_out, int64_t out_stride, int64_t *n_out, void *hip_stream)
{
    if (!r) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (n_out) *n_out = 0;
    int64_t emit = 0;
    if (int st = sinc_flush_check(r, d_out != nullptr, out_stride, &emit)) return st;
    if (emit > 0) {
        SYLDET_HIP(hipSetDevice(r->device));
        // the row ends at N: no pushed rows, no carry
        SYLDET_HIP(launch_sinc_stream_push(r->d_hist[r->cur], r->d_hist[r->cur ^ 1], r->L, nullptr, 0, 0, r->n_in_total, d_out, out_stride,
                                           r->n_out_total, emit, r->channels, r->rate_in, r->rate_out, r->H, (float)r->s, r->d_table,
                                           r->entries, (hipStream_t)hip_stream));
    }
    r->n_out_total += emit;
    r->finished = true;
    if (n_out) *n_out = emit;
    return SYLDET_OK;
}

int syldet_sinc_resample(syldet_sinc_resampler_t *r, const float *in, int64_t n_in, int64_t in_stride, float *out, int64_t out_stride,
                         int64_t *n_out)
{
    if (!r) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (n_out) *n_out = 0;
    int64_t emit = 0;
    if (int st = sinc_push_check(r, in != nullptr, n_in, in_stride, out != nullptr, out_stride, &emit)) return st;
    if (n_in == 0) return SYLDET_OK;
    SYLDET_HIP(hipSetDevice(r->device));
    if (int st = sinc_stage(r, n_in, emit)) return st;
    const size_t C = (size_t)r->channels;
    SYLDET_HIP(hipMemcpy2DAsync(r->d_in, (size_t)n_in * sizeof(float), in, (size_t)(C > 1 ? in_stride : n_in) * sizeof(float),
                                (size_t)n_in * sizeof(float), C, hipMemcpyHostToDevice, r->stream));
    if (int st = sinc_push_device<float>(r, r->d_in, n_in, n_in, r->d_out, emit, n_out, r->stream)) return st;
    if (emit > 0)
        SYLDET_HIP(hipMemcpy2DAsync(out, (size_t)(C > 1 ? out_stride : emit) * sizeof(float), r->d_out, (size_t)emit * sizeof(float),
                                    (size_t)emit * sizeof(float), C, hipMemcpyDeviceToHost, r->stream));
    SYLDET_HIP(hipStreamSynchronize(r->stream));
    return SYLDET_OK;
}

int syldet_sinc_resampler_flush(syldet_sinc_resampler_t *r, float *out, int64_t out_stride, int64_t *n_out)
{
    if (!r) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (n_out) *n_out = 0;
    int64_t emit = 0;
    if (int st = sinc_flush_check(r, out != nullptr, out_stride, &emit)) return st;
    SYLDET_HIP(hipSetDevice(r->device));
    if (int st = sinc_stage(r, 0, emit)) return st;
    if (int st = syldet_sinc_resampler_flush_device(r, r->d_out, emit, n_out, r->stream)) return st;
    const size_t C = (size_t)r->channels;
    if (emit > 0)
        SYLDET_HIP(hipMemcpy2DAsync(out, (size_t)(C > 1 ? out_stride : emit) * sizeof(float), r->d_out, (size_t)emit * sizeof(float),
                                    (size_t)emit * sizeof(float), C, hipMemcpyDeviceToHost, r->stream));
    SYLDET_HIP(hipStreamSynchronize(r->stream));
    return SYLDET_OK;
}

void syldet_sinc_defaults(int32_t *zero_crossings, double *beta, double *rolloff)
{
    if (zero_crossings) *zero_crossings = 32;
    if (beta) *beta = 12.0;
    if (rolloff) *rolloff = 0.9;
}

double syldet_sinc_coefficient(double t, double rate_in, double rate_out, int32_t zero_crossings, double beta, double rolloff)
{
    double s = 0.0, H = 0.0;
    if (sinc_design(rate_in, rate_out, zero_crossings, beta, rolloff, &s, &H)) return std::nan("");
    if (t != t) return t;
    const double u = t / H;
    if (!(std::fabs(t) < H)) return 0.0;
    return s * sinc_pi(s * t) * bessel_i0(beta * std::sqrt(1.0 - u * u)) / bessel_i0(beta);
}

int64_t syldet_sinc_taps(double rate_in, double rate_out, int32_t zero_crossings, double rolloff)
{
    double s = 0.0, H = 0.0;
    if (sinc_design(rate_in, rate_out, zero_crossings, 0.0, rolloff, &s, &H)) return -1;
    return 2 * (int64_t)std::floor(H) + 1;
}

int syldet_convert_rate_sinc_device(const float *d_in, int64_t n_in, int64_t in_stride, int32_t n_channels, double rate_in,
                                    double rate_out, int32_t zero_crossings, double beta, double rolloff, float *d_out,
                                    int64_t out_stride, int64_t *n_out, void *hip_stream)
{
    return convert_rate_sinc<float>(d_in, n_in, in_stride, n_channels, rate_in, rate_out, zero_crossings, beta, rolloff, d_out,
                                    out_stride, n_out, hip_stream);
}

int syldet_convert_rate_sinc_device_s16(const int16_t *d_in, int64_t n_in, int64_t in_stride, int32_t n_channels, double rate_in,
                                        double rate_out, int32_t zero_crossings, double beta, double rolloff, float *d_out,
                                        int64_t out_stride, int64_t *n_out, void *hip_stream)
{
    return convert_rate_sinc<int16_t>(d_in, n_in, in_stride, n_channels, rate_in, rate_out, zero_crossings, beta, rolloff, d_out,
                                      out_stride, n_out, hip_stream);
}

int syldet_deinterleave_device_s16(const int16_t *d_interleaved, int64_t n_frames, int32_t total_channels, int32_t n_channels,
                                   int16_t *d_out, int64_t out_stride, void *hip_stream)
{
    if (n_frames < 0 || total_channels <= 0 || n_channels <= 0 || n_channels > total_channels)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "channel selection outside the interleaved layout");
    if (n_frames == 0) return SYLDET_OK;
    if (!d_interleaved || !d_out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (out_stride < n_frames) return fail(SYLDET_ERR_INVALID_ARGUMENT, "out_stride must be >= n_frames");
    SYLDET_HIP(launch_deinterleave_s16(d_interleaved, n_frames, total_channels, n_channels, d_out, out_stride, (hipStream_t)hip_stream));
    return SYLDET_OK;
}

int syldet_deinterleave_device(const float *d_interleaved, int64_t n_frames, int32_t total_channels, int32_t first_channel,
                               int32_t n_channels, float *d_out, int64_t out_stride, void *hip_stream)
{
    if (n_frames < 0 || total_channels <= 0 || first_channel < 0 || n_channels <= 0 || first_channel + n_channels > total_channels)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "channel selection outside the interleaved layout");
    if (n_frames == 0) return SYLDET_OK;
    if (!d_interleaved || !d_out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (n_channels > 1 && out_stride < n_frames) return fail(SYLDET_ERR_INVALID_ARGUMENT, "out_stride must be >= n_frames");
    SYLDET_HIP(launch_deinterleave(d_interleaved, n_frames, total_channels, first_channel, n_channels, d_out, out_stride,
                                   (hipStream_t)hip_stream));
    return SYLDET_OK;
}

int syldet_pack_flags_device(const uint8_t *d_flags, int64_t rows, int64_t row_len, uint8_t *d_bits, void *hip_stream)
{
    if (rows < 0 || row_len < 0 || rows > 65535) return fail(SYLDET_ERR_INVALID_ARGUMENT, "rows must be in [0, 65535], row_len >= 0");
    if (rows == 0 || row_len == 0) return SYLDET_OK;
    if (!d_flags || !d_bits) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL buffer");
    SYLDET_HIP(launch_pack_flags(d_flags, rows, row_len, d_bits, (hipStream_t)hip_stream));
    return SYLDET_OK;
}

int syldet_unpack_flags_device(const uint8_t *d_bits, int64_t rows, int64_t row_len, uint8_t *d_flags, void *hip_stream)
{
    if (rows < 0 || row_len < 0 || rows > 65535) return fail(SYLDET_ERR_INVALID_ARGUMENT, "rows must be in [0, 65535], row_len >= 0");
    if (rows == 0 || row_len == 0) return SYLDET_OK;
    if (!d_flags || !d_bits) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL buffer");
    SYLDET_HIP(launch_unpack_flags(d_bits, rows, row_len, d_flags, (hipStream_t)hip_stream));
    return SYLDET_OK;
}

}  // extern "C"
