/*
 * syldet.h -- C ABI of libsyldet, the MI355X (gfx950) batched syllable-detection engine.
 *
 * This is the drop-in boundary for ONE path of gardner-lab/syllable-detector-swift:
 *   CircularShortTimeFourierTransform.extractPower  -> band slice -> sliding timeRange window
 *   -> NeuralNet.apply -> threshold,   as driven by SyllableDetector.processNewValue.
 *
 * The reference has no FFI for this path (the arithmetic is inline Swift calling Apple
 * Accelerate); its only C boundary is Common/Common-Bridging-Header.h:5, which exposes
 * TPCircularBuffer.h to Swift.  libsyldet is bound the same way (one more #include in
 * that bridging header), and every entry point below names the
 * reference interface (file:line, relative to the reference root) it stands in for.
 *
 * Conventions
 *   - plain C types only; the library copies every configuration array at create time;
 *     callers own all input/output buffers; the library owns its device memory;
 *   - return value: SYLDET_OK (0) or a negative syldet_status_t.  Where the reference
 *     calls fatalError (ring overflow, shape mismatch, bad FFT size) or throws
 *     ParseError, this ABI returns a status instead of aborting the host; data
 *     availability is reported as 1/0 like processNewValue's Bool;
 *   - `*_device` entry points take device pointers and a hipStream_t (passed as void*)
 *     and are asynchronous on that stream; the others take host pointers and block;
 *   - channels are independent detectors (Processor.swift:57-59: one SyllableDetector
 *     per channel; main.swift:86-89: one per track); batch layouts are channel-major;
 *   - threading: one producer (append) + one consumer (process/read) per channel, as
 *     TPCircularBuffer.h:14 guarantees in the reference (append never locks; it allocates
 *     once, on a channel's first samples); the host-pointer batch calls and the streaming
 *     consumers of one handle serialise on its staging buffers; the *_device batch calls are
 *     not re-entrant on one handle, and two of them must not be in flight at once on different
 *     streams either (a handle owns one scratch set and one work list of the precision guard:
 *     enqueue a handle's calls on one stream, or use a handle per stream); distinct handles are
 *     independent.
 *   - there is NO CPU fallback: without a gfx950 device create fails with
 *     SYLDET_ERR_NO_DEVICE.
 */
#ifndef SYLDET_H
#define SYLDET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SYLDET_ABI_VERSION 1

typedef enum {
    SYLDET_OK = 0,
    SYLDET_ERR_INVALID_ARGUMENT   = -1,  /* NULL pointer, negative size, bad enum                        */
    SYLDET_ERR_FFT_SIZE           = -2,  /* CircularShortTimeFourierTransform.swift:82-88 fatalError     */
    SYLDET_ERR_OVERLAP            = -3,  /* CircularShortTimeFourierTransform.swift:76-78 fatalError     */
    SYLDET_ERR_FREQ_RANGE         = -4,  /* SyllableDetector.swift:46-48 fatalError                      */
    SYLDET_ERR_INPUT_MISMATCH     = -5,  /* SyllableDetector.swift:52-55 fatalError                      */
    SYLDET_ERR_THRESHOLD_MISMATCH = -6,  /* SyllableDetector.swift:58-60 fatalError                      */
    SYLDET_ERR_LAYER_SHAPE        = -7,  /* NeuralNet.swift:244-254, :341-349 fatalError                 */
    SYLDET_ERR_BUFFER_FULL        = -8,  /* CircularShortTimeFourierTransform.swift:199 "Insufficient space on buffer." */
    SYLDET_ERR_NO_DEVICE          = -9,  /* no gfx950 device / HIP runtime failure at create             */
    SYLDET_ERR_DEVICE             = -10, /* HIP error during a call (message via syldet_last_error)      */
    SYLDET_ERR_OUT_OF_MEMORY      = -11,
    SYLDET_ERR_PARSE_OPEN         = -20, /* ParseError.unableToOpenPath, SyllableDetectorConfig.swift:51 */
    SYLDET_ERR_PARSE_MISSING      = -21, /* ParseError.missingValue     :52                              */
    SYLDET_ERR_PARSE_INVALID      = -22, /* ParseError.invalidValue     :53                              */
    SYLDET_ERR_PARSE_LENGTH       = -23, /* ParseError.mismatchedLength :54                              */
    SYLDET_ERR_UNSUPPORTED        = -30
} syldet_status_t;

/* WindowType, CircularShortTimeFourierTransform.swift:12-29.  SyllableDetector always
 * selects hamming (SyllableDetector.swift:43); the others are the STFT class's options. */
typedef enum { SYLDET_WINDOW_NONE = 0, SYLDET_WINDOW_HAMMING = 1, SYLDET_WINDOW_HANNING = 2,
               SYLDET_WINDOW_BLACKMAN = 3 } syldet_window_t;
/* SyllableDetectorConfig.Scaling, SyllableDetectorConfig.swift:13-30 */
typedef enum { SYLDET_SCALING_LINEAR = 0, SYLDET_SCALING_LOG = 1, SYLDET_SCALING_DB = 2 } syldet_scaling_t;
/* extractPower (|X|, what the detector uses) vs extractMagnitude (|X|^2),
 * CircularShortTimeFourierTransform.swift:280 / :221 (the names are as in the reference) */
typedef enum { SYLDET_SPECTRUM_POWER = 0, SYLDET_SPECTRUM_MAGNITUDE = 1 } syldet_spectrum_t;
/* processing functions accepted by SyllableDetectorConfig.swift:133-151 (inputs) and
 * :158-167 (outputs: mapminmax, mapstd only)                                            */
typedef enum { SYLDET_FN_L2NORMALIZE = 0, SYLDET_FN_NORMALIZE = 1, SYLDET_FN_NORMALIZESTD = 2,
               SYLDET_FN_MAPMINMAX = 3, SYLDET_FN_MAPSTD = 4 } syldet_fn_kind_t;
/* transfer functions, SyllableDetectorConfig.swift:250-256 / NeuralNet.swift:185-228 */
typedef enum { SYLDET_TF_TANSIG = 0, SYLDET_TF_LOGSIG = 1, SYLDET_TF_PURELIN = 2,
               SYLDET_TF_SATLIN = 3 } syldet_transfer_t;
/* which outputs raise the detection flag: output 0 (SyllableDetector.lastDetected,
 * SyllableDetector.swift:27-31) or any output (CLI, TrackDetector.swift:72-77)          */
typedef enum { SYLDET_RULE_FIRST = 0, SYLDET_RULE_ANY = 1 } syldet_rule_t;

/* MapMinMax / MapStd parameters, NeuralNet.swift:111-182 (count = vector length; unused
 * and 0 for the parameter-free functions)                                               */
typedef struct {
    int32_t kind;            /* syldet_fn_kind_t */
    int32_t count;
    const float *x_offsets;
    const float *gains;
    float y;                 /* yMin (mapminmax) / yMean (mapstd) */
} syldet_fn_t;

/* NeuralNetLayer, NeuralNet.swift:329-378.  weights row-major [outputs][inputs]
 * (vDSP_mmul M=outputs, P=inputs at :368; convert_to_text.m:202).                        */
typedef struct {
    int32_t inputs, outputs;
    int32_t transfer;        /* syldet_transfer_t */
    const float *weights;
    const float *biases;
} syldet_layer_t;

/* SyllableDetectorConfig, SyllableDetectorConfig.swift:11-45 (+ the STFT options the
 * detector fixes).  All arrays are copied by syldet_create.                              */
typedef struct {
    double sampling_rate;            /* samplingRate  */
    int32_t fourier_length;          /* fourierLength */
    int32_t window_length;           /* windowLength  */
    int32_t window_overlap;          /* windowOverlap; negative = gap between windows */
    double freq_lo, freq_hi;         /* freqRange     */
    int32_t time_range;              /* timeRange     */
    int32_t scaling;                 /* syldet_scaling_t  */
    int32_t window;                  /* syldet_window_t; the detector uses SYLDET_WINDOW_HAMMING */
    int32_t spectrum;                /* syldet_spectrum_t; the detector uses SYLDET_SPECTRUM_POWER */
    int32_t rule;                    /* syldet_rule_t     */
    int32_t n_input_fns;
    const syldet_fn_t *input_fns;    /* net.inputProcessing, applied in order */
    int32_t n_layers;
    const syldet_layer_t *layers;    /* net.layers */
    int32_t n_output_fns;
    const syldet_fn_t *output_fns;   /* net.outputProcessing, applied in order as reverse maps */
    int32_t n_thresholds;
    const double *thresholds;        /* thresholds (Double) */
} syldet_config_t;

/* Derived geometry (what SyllableDetector.init computes, SyllableDetector.swift:42-60). */
typedef struct {
    int32_t gap, overlap, hop;       /* CircularShortTimeFourierTransform.swift:66-73; hop = gap + W - overlap */
    int32_t f0, f1;                  /* frequencyIndexRange, :166-191 */
    int32_t bins;                    /* F = f1 - f0 */
    int32_t inputs;                  /* F * timeRange == net.inputs */
    int32_t outputs;                 /* net.outputs */
    int32_t first_index;             /* sample number of evaluation 0, TrackDetector.swift:39-42 */
    int32_t engine;                  /* which kernel family create selected (syldet_engine_t) */
} syldet_geometry_t;

/* SYLDET_ENGINE_WIDE_BF16: two-layer networks with a wide hidden layer (BASELINE: 4096 units) evaluated as a bf16
 * MFMA GEMM over thousands of evaluations, fp32 accumulate.  Inputs and first-layer weights are rounded to bf16, so
 * results agree with the fp32 engines to ~1e-3, not 1e-5: opt-in only, never selected by AUTO.                   */
typedef enum { SYLDET_ENGINE_AUTO = 0, SYLDET_ENGINE_GENERIC = 1, SYLDET_ENGINE_FUSED = 2,
               SYLDET_ENGINE_WIDE_BF16 = 3 } syldet_engine_t;

typedef struct syldet syldet_t;

/* ---- library ---- */
int         syldet_abi_version(void);
const char *syldet_strerror(int status);
/* message of the last failing call on this thread (HIP error text, parse key, ...) */
const char *syldet_last_error(void);

/* ---- configuration file ----
 * SyllableDetectorConfig.init(fromTextFile:), SyllableDetectorConfig.swift:170-277.
 * On success *out owns every array it points to; free with syldet_config_free.
 * window/spectrum/rule are set to the detector's fixed choices (hamming, power, first). */
int  syldet_config_load_text(const char *path, syldet_config_t **out);
void syldet_config_free(syldet_config_t *cfg);
/* the same validation SyllableDetector.init performs, without touching a device */
int  syldet_config_geometry(const syldet_config_t *cfg, syldet_geometry_t *out);
/* CircularShortTimeFourierTransform.frequencyIndexRange, :166-191 (1 = range found, 0 = nil) */
int  syldet_frequency_index_range(int32_t fourier_length, double sampling_rate, double lo, double hi,
                                  int32_t *f0, int32_t *f1);
/* WindowType.createWindow, :19-28 */
int  syldet_make_window(int32_t window, int32_t length, float *out);

/* ---- detector bank ----
 * SyllableDetector.init(config:), SyllableDetector.swift:37-74, for n_channels
 * independent channels on HIP device `device`.  engine: SYLDET_ENGINE_AUTO unless a
 * test wants a specific kernel family.                                                  */
int syldet_create(const syldet_config_t *cfg, int32_t n_channels, int32_t device, int32_t engine,
                  syldet_t **out);
/* ---- one bank, a network per channel ----
 * ProcessorBase.init (Processor.swift:50-86) builds one SyllableDetector per channel from that channel's own configuration
 * (ViewControllerProcessor.loadNetworkForRow, ViewControllerProcessor.swift:222-276, loads one file per row): channel c of
 * this handle runs network cfgs[channel_net[c]].  All networks must be COMPATIBLE (syldet_config_compatible): they share the
 * framing and the shape of the chain -- sampling_rate, fourier_length, window_length, window_overlap, time_range, the derived
 * band (f0, f1) (freq_lo / freq_hi may differ where they give the same bins), scaling, window, spectrum, rule, the number and
 * kinds of the input and output functions, the number of layers and each layer's inputs, outputs and transfer, n_thresholds.
 * Weights, biases, the functions' parameters (x_offsets, gains, y) and thresholds may differ -- networks trained with the same
 * settings for different birds.  Configurations that are not compatible need a handle each.
 * Statuses: SYLDET_ERR_UNSUPPORTED for incompatible networks (syldet_last_error names the field), SYLDET_ERR_INVALID_ARGUMENT for
 * a NULL pointer, n_nets < 1 or a channel_net entry outside [0, n_nets); a network no channel uses is allowed.  These checks run
 * before any device is touched.  Everything is copied at create time.
 * Engines: AUTO runs the fold kernel (the symmetric-fold fused kernel) when every network's own AUTO handle would, and otherwise
 * the generic engine exactly as SYLDET_ENGINE_GENERIC has it; FUSED is the fold kernel or SYLDET_ERR_UNSUPPORTED where it does
 * not take the shape; GENERIC the generic engine; WIDE_BF16 is SYLDET_ERR_UNSUPPORTED.  n_nets == 1 makes a syldet_create handle.
 * Every other entry point works on the handle unchanged and answers each channel from its own network.                    */
int syldet_create_multi(const syldet_config_t *const *cfgs, int32_t n_nets, const int32_t *channel_net, int32_t n_channels,
                        int32_t device, int32_t engine, syldet_t **out);
/* 1 = a and b may share one handle, 0 = they may not (*field, if field is not NULL, names the first difference: a static
 * string such as "time_range" or "layers.outputs"), < 0 = status (NULL argument, or a configuration syldet_create refuses) */
int syldet_config_compatible(const syldet_config_t *a, const syldet_config_t *b, const char **field);

/* ---- one bank, networks of different bands and shapes (a mixed bank) ----
 * The same contract as syldet_create_multi -- channel c runs network cfgs[channel_net[c]] -- for networks that need only share
 * the EVALUATION CLOCK (syldet_config_same_clock): sampling_rate, window_length, window_overlap, time_range and n_thresholds
 * (the number of outputs).  Those fix gap, hop, first_index, syldet_count_evals and the [C][E][n_out] output layout, so every
 * batch, streaming and detection entry point keeps its shapes.  Everything else may differ: fourier_length, the band (and so
 * the bins and the first layer's inputs), scaling, window, spectrum, rule, the processing functions, the layers and all values
 * -- ProcessorBase's rows each load their own trained file (Processor.swift:50-86, ViewControllerProcessor.swift:222-276).
 * The library partitions the networks into CLASSES of compatible ones (syldet_config_compatible); each class runs exactly as a
 * syldet_create_multi handle of its networks would -- the same engine choice under AUTO / GENERIC / FUSED, the same kernels,
 * the same arithmetic -- reading the caller's rows where they are and writing each channel's results in place.  A batch call
 * launches the classes one after another on the caller's stream; a streaming drain makes one H2D copy, the classes' launches,
 * one D2H copy and one synchronisation per evaluation-count group.  Classes that would want an engine without a multi-network
 * form (the wide engine, the matrix-core network stages) run on the generic engine, as syldet_create_multi does.
 * Statuses: SYLDET_ERR_INVALID_ARGUMENT for a NULL pointer, n_nets < 1 or a channel_net entry outside [0, n_nets); a
 * configuration syldet_create refuses, that status; SYLDET_ERR_UNSUPPORTED for a clock mismatch (syldet_last_error names the
 * field), for WIDE_BF16, and for FUSED when a class does not take the fold kernel.  All of these before any device is touched.
 * All networks compatible: exactly a syldet_create_multi handle (n_nets == 1: a syldet_create handle).
 * syldet_get_geometry: the shared fields as usual; f0, f1, bins, inputs and engine are -1 where the classes differ
 * (syldet_channel_geometry has each channel's own).  syldet_spectrogram* on a bank of more than one class is
 * SYLDET_ERR_UNSUPPORTED (the columns are ragged).  Every other entry point works unchanged and answers each channel from its own
 * network; syldet_fixup_stats sums the classes' recomputations.                                                             */
int syldet_create_mixed(const syldet_config_t *const *cfgs, int32_t n_nets, const int32_t *channel_net, int32_t n_channels,
                        int32_t device, int32_t engine, syldet_t **out);
/* 1 = a and b share the evaluation clock and may share a mixed bank, 0 = they may not (*field names the first difference:
 * "sampling_rate", "window_length", "window_overlap", "time_range" or "n_thresholds"), < 0 = status, as
 * syldet_config_compatible */
int syldet_config_same_clock(const syldet_config_t *a, const syldet_config_t *b, const char **field);
/* The geometry of channel `channel`'s own network (its class's, on a mixed bank; the handle's, on any other) */
int syldet_channel_geometry(const syldet_t *h, int32_t channel, syldet_geometry_t *out);

int syldet_destroy(syldet_t *h);
int syldet_get_geometry(const syldet_t *h, syldet_geometry_t *out);
int32_t syldet_channels(const syldet_t *h);

/* frames J = floor((S - gap - W)/hop) + 1 and evaluations E = J - T + 1 that S samples
 * per channel yield (extractPower's availability rule :286-288 + consume :299-302;
 * processNewValue's :164-178)                                                            */
int64_t syldet_count_frames(const syldet_t *h, int64_t n_samples);
int64_t syldet_count_evals(const syldet_t *h, int64_t n_samples);

/* ---- batch: the whole of `while detector.processNewValue() {...}` for every channel ----
 * (TrackDetector.swift:62-77 / Processor.swift:136-141).
 * samples  [C][channel_stride] fp32, the first n_samples of each row are used;
 * outputs  [C][E][outputs]    fp32  = lastOutputs after each evaluation;
 * flags    [C][E]             u8    = Double(out) >= threshold under cfg.rule;
 * Either output pointer may be NULL.                                                     */
int syldet_run_device(syldet_t *h, const float *d_samples, int64_t n_samples, int64_t channel_stride,
                      float *d_outputs, uint8_t *d_flags, void *hip_stream);
int syldet_run(syldet_t *h, const float *samples, int64_t n_samples, int64_t channel_stride,
               float *outputs, uint8_t *flags);
/* 16-bit PCM: samples [C][channel_stride] int16 (strides count elements), sample x meaning x / 32768 = float(x) * 2^-15 --
 * the value a WAV reader or the reference's AVFoundation reader (32-bit float delivery) gives for it.  Each result is
 * bit-identical to the fp32 twin's on the same handle fed float(x) * 2^-15 with the same strides: outputs, flags, detections and
 * syldet_fixup_stats' item counts, on every engine and bank kind; the argument checks and statuses are the fp32 twin's, made
 * before any device is touched.  Read natively (2 bytes a sample) by the fold kernel's twice-folded form on the plain ring
 * with up to 4 hidden units -- the reference's 256-point framing wherever the plan keeps the plain sample ring (hop 128's
 * staggered chunks and the padded ring of other multiples of 64 do not), any chain the fold kernel takes, plain, multi-network
 * and mixed banks -- where the rows are whole 4-byte words (a 4-byte aligned base, an even stride); the exact recomputation
 * reads them too.  Every other shape and layout is read once into a packed fp32 copy
 * (syldet_timings lists "widen_s16_kernel", at most once a call) and runs the fp32 kernels on it.  That copy, C x S x 4 bytes,
 * is scratch the handle keeps until it is destroyed and the fp32 call does not need: an s16 call may fail with
 * SYLDET_ERR_OUT_OF_MEMORY where its fp32 twin succeeds.  syldet_run_s16 cuts the recording into the stages syldet_run would
 * use and copies int16: half the bytes cross the bus.                                                                       */
int syldet_run_device_s16(syldet_t *h, const int16_t *d_samples, int64_t n_samples, int64_t channel_stride,
                          float *d_outputs, uint8_t *d_flags, void *hip_stream);
int syldet_run_s16(syldet_t *h, const int16_t *samples, int64_t n_samples, int64_t channel_stride,
                   float *outputs, uint8_t *flags);

/* syldet_run cuts a long recording along time into stages of about 256 MiB of input and overlaps the H2D copy of the next
 * stage with the kernel of this one and the D2H copy of the last (device staging: two stages, whatever the length).
 * The copies read and write the caller's rows in place: buffers from syldet_host_alloc are page-locked, their copies
 * truly asynchronous; ordinary buffers work too (the runtime pins the pages of each copy as it goes).  TPCircularBufferInit (TPCircularBuffer.c:43-124) is the reference's
 * allocation of the buffer audio is produced into; this is its counterpart for a host that feeds a GPU.                 */
int syldet_host_alloc(size_t bytes, void **out);
int syldet_host_free(void *p);

/* the spectrogram columns the detector feeds its network, [C][J][bins] fp32
 * (processFourierData, SyllableDetector.swift:134-151; linear values, before scaling)    */
int syldet_spectrogram_device(syldet_t *h, const float *d_samples, int64_t n_samples, int64_t channel_stride,
                              float *d_columns, void *hip_stream);
int syldet_spectrogram(syldet_t *h, const float *samples, int64_t n_samples, int64_t channel_stride,
                       float *columns);

/* detection sample numbers with debounce, TrackDetector.swift:39-43,:65-100:
 * idx_e = first_index + e*hop; emit iff flag && debounce_until < idx_e, then
 * debounce_until = idx_e + Int(debounce_seconds * samplingRate).
 * indices [C][capacity] int64 (first counts[c] valid), counts [C] int64 (may exceed
 * capacity: the number that would have been written).                                    */
int syldet_detections_device(syldet_t *h, const uint8_t *d_flags, int64_t n_evals, double debounce_seconds,
                             int64_t *d_indices, int64_t capacity, int64_t *d_counts, void *hip_stream);
int syldet_detections(syldet_t *h, const uint8_t *flags, int64_t n_evals, double debounce_seconds,
                      int64_t *indices, int64_t capacity, int64_t *counts);

/* ---- the Simulator's output track (SyllableDetector/ViewControllerSimulator.swift:251-344) ----
 * simulateNetwork writes a second audio file of the recording's length and rate whose samples are output 0 as a fraction of
 * its threshold, held from one evaluation to the next (:322-343).  With D = first_index (the Simulator's nextCount, :251-254,
 * TrackDetector.swift:39-42's number) and hop = windowLength - windowOverlap (the hold, :331):
 *   v[e]     = clamp01(out[e][output] / Float(thresholds[output]))     fp32 division (:322); clamp01 is two comparisons
 *                                                                      (:323-328): v > 1 -> 1, v < 0 -> 0, else unchanged --
 *                                                                      NaN stays NaN, x / 0 is 1 or 0 by its sign
 *   trace[s] = 0 for s < D;  v[(s - D) / hop] for D <= s < D + n_evals hop;  0 beyond
 * d_outputs [C][n_evals][outputs] as syldet_run_device wrote them; d_trace [C][trace_stride], the first n_samples of each row
 * are written and nothing else.  n_evals and n_samples are independent (with n_evals = syldet_count_evals(n_samples) the
 * last hold reaches n_samples or beyond: no sample lies behind it).  `output` picks the output (0: the Simulator's).  On
 * syldet_create_multi / syldet_create_mixed banks channel c divides by its own network's threshold.  The fp32 form is the
 * reference's, bit for bit.  The 16-bit form is THIS LIBRARY'S convention (the reference hands its floats to AVFoundation's
 * 16-bit file writer, :206-218, whose rounding is not specified):
 *   q = (int16) rint(v * 32767), ties to even, computed in fp32 without contraction, NaN -> 0
 * so 0 <-> 0 and the threshold and everything above it <-> 32767.  One kernel launch a call (syldet_timings lists it as
 * "trace_kernel", the frame-major form of two or more channels as "trace_interleaved_s16_kernel"); the [C] table of
 * Float(thresholds[output]) is made on the first call for that output (a blocking copy) and kept by the handle.
 * Statuses, before any device is touched: SYLDET_ERR_INVALID_ARGUMENT for a NULL handle or pointer, n_evals < 0, n_samples < 0,
 * trace_stride < n_samples, output outside [0, outputs).  n_samples == 0 writes nothing; n_evals == 0 writes rows of zeros.
 * The device forms follow the handle's rule of one stream at a time.                                                        */
int syldet_trace_device(syldet_t *h, const float *d_outputs, int64_t n_evals, int32_t output,
                        float *d_trace, int64_t n_samples, int64_t trace_stride, void *hip_stream);
int syldet_trace_device_s16(syldet_t *h, const float *d_outputs, int64_t n_evals, int32_t output,
                            int16_t *d_trace, int64_t n_samples, int64_t trace_stride, void *hip_stream);
/* d_frames [n_samples][C] int16: what a 16-bit WAV of C tracks stores (simulateNetwork writes 16-bit linear PCM, :187-218;
 * here every track at once); equal to syldet_trace_device_s16's rows, transposed (one channel: the planar kernel)         */
int syldet_trace_interleaved_device_s16(syldet_t *h, const float *d_outputs, int64_t n_evals, int32_t output,
                                        int16_t *d_frames, int64_t n_samples, void *hip_stream);
/* host pointers, blocking (as syldet_detections is to syldet_detections_device) */
int syldet_trace(syldet_t *h, const float *outputs, int64_t n_evals, int32_t output,
                 float *trace, int64_t n_samples, int64_t trace_stride);
int syldet_trace_s16(syldet_t *h, const float *outputs, int64_t n_evals, int32_t output,
                     int16_t *trace, int64_t n_samples, int64_t trace_stride);

/* ---- the level meters of a row (SyllableDetector/Processor.swift:111-113, :138, :158-184; SummaryStat.swift) ----
 * ProcessorBase keeps two StatMax statistics per row, read and reset by a 0.1 s timer (ViewControllerProcessor.swift:57,
 * :184-189, :278-284): the input meter takes Double(sum of squares) / Double(length) of every callback buffer (its reading is the
 * square root of the greatest: an RMS), the output meter Double(lastOutputs[0]) of every evaluation.
 * StatMax takes its first value as it is and a later one only if it is greater: a reading is NaN if its first value is NaN, and
 * otherwise the greatest (the first of equal ones) of its values that are not NaN.
 * The sum of squares is THIS LIBRARY'S convention (vDSP_svesq's order is not specified), sum_squares_tree(x, n): every square
 * x[i] * x[i] rounded to fp32 on its own, the squares added as a balanced binary tree in index order over next_pow2(n) slots,
 * the slots past n holding +0, every addition rounded to fp32, no multiply-add contraction.  (Padding to a longer power of two
 * gives the same bits.)  syldet_sum_squares is that function on the host.
 * The batch form of the timer, for buffer_length L (a power of two, 8 <= L <= 4096; the reference's default is 32,
 * AudioInterface.swift:342, :474) and buffers_per_reading P >= 1: buffer b is samples [b L, min((b + 1) L, S)) -- B = ceil(S / L),
 * the last one may be short and divides by its own length --, reading m is buffers [m P, (m + 1) P), M = ceil(B / P) =
 * syldet_levels_count.
 *   d_mean_square [C][M] fp64   the StatMax of the buffers' mean squares (the RMS is its sqrt; the host forms below return that)
 *   d_levels      [C][M] fp32   the StatMax of out[e][output] over the evaluations the reading's buffers make available:
 *                               [min(ce(min(m P L, S)), n_evals), min(ce(min((m + 1) P L, S)), n_evals)), ce = syldet_count_evals
 *                               (syldet_levels_eval_range); 0 for a reading without one (the table's `?? 0.0`)
 * int16 samples mean float(x) * 2^-15 and give the fp32 form's bits.  syldet_timings lists "levels_in_kernel", "levels_fold_kernel"
 * (where a reading crosses workgroups) and "levels_out_kernel"; the interleaved forms de-interleave into the handle's planar
 * scratch first (total_channels == syldet_channels(h), as syldet_run_interleaved*).
 * Statuses, before any device is touched: SYLDET_ERR_INVALID_ARGUMENT for a NULL handle or pointer, negative counts, a stride
 * below n_samples, output outside [0, outputs), an L that is not a power of two in [8, 4096], P < 1.  n_samples == 0 writes
 * nothing.  The device forms follow the handle's rule of one stream at a time.  Plain, multi-network and mixed banks alike.  */
int64_t syldet_levels_count(int64_t n_samples, int32_t buffer_length, int64_t buffers_per_reading);   /* M; -1 for bad arguments */
float   syldet_sum_squares(const float *x, int64_t n);
/* the evaluations [*first, *first + *count) of reading `reading` (in [0, M)) for n_evals evaluations of n_samples samples */
int syldet_levels_eval_range(const syldet_t *h, int64_t n_samples, int64_t n_evals, int32_t buffer_length,
                             int64_t buffers_per_reading, int64_t reading, int64_t *first, int64_t *count);
int syldet_levels_device(syldet_t *h, const float *d_samples, int64_t n_samples, int64_t channel_stride,
                         int32_t buffer_length, int64_t buffers_per_reading, double *d_mean_square, void *hip_stream);
int syldet_levels_device_s16(syldet_t *h, const int16_t *d_samples, int64_t n_samples, int64_t channel_stride,
                             int32_t buffer_length, int64_t buffers_per_reading, double *d_mean_square, void *hip_stream);
int syldet_levels_interleaved_device(syldet_t *h, const float *d_interleaved, int64_t n_frames, int32_t total_channels,
                                     int32_t buffer_length, int64_t buffers_per_reading, double *d_mean_square, void *hip_stream);
int syldet_levels_interleaved_device_s16(syldet_t *h, const int16_t *d_interleaved, int64_t n_frames, int32_t total_channels,
                                         int32_t buffer_length, int64_t buffers_per_reading, double *d_mean_square, void *hip_stream);
int syldet_output_levels_device(syldet_t *h, const float *d_outputs, int64_t n_evals, int32_t output, int64_t n_samples,
                                int32_t buffer_length, int64_t buffers_per_reading, float *d_levels, void *hip_stream);
/* host pointers, blocking (as syldet_trace is to syldet_trace_device); rms [C][M]: the square roots (std::sqrt on the host) */
int syldet_levels(syldet_t *h, const float *samples, int64_t n_samples, int64_t channel_stride,
                  int32_t buffer_length, int64_t buffers_per_reading, double *rms);
int syldet_levels_s16(syldet_t *h, const int16_t *samples, int64_t n_samples, int64_t channel_stride,
                      int32_t buffer_length, int64_t buffers_per_reading, double *rms);
int syldet_output_levels(syldet_t *h, const float *outputs, int64_t n_evals, int32_t output, int64_t n_samples,
                         int32_t buffer_length, int64_t buffers_per_reading, float *levels);
/* Streaming: getInputForChannel / getOutputForChannel (Processor.swift:158-184).  Off until syldet_meters_enable(h, 1) (a handle
 * that never enables them does what it always did; enabling or disabling clears both statistics).  When on, every syldet_append*
 * call that succeeds with n > 0 is one buffer per channel (sum_squares_tree over the call's samples -- for the s16 appends over
 * the converted values -- divided by the call's length), and every evaluation syldet_process_new_value / syldet_seen_syllable
 * makes lastOutputs writes output 0.  The getters read and reset (*has_value = 0 and *rms / *level = 0 where nothing was
 * written: the reference's nil); they may be called from any thread beside the producer and the consumer (a small lock per
 * channel: no value is lost between a write and a read-and-reset).                                                        */
int syldet_meters_enable(syldet_t *h, int enable);
int syldet_input_level(syldet_t *h, int32_t channel, double *rms, int32_t *has_value);
int syldet_output_level(syldet_t *h, int32_t channel, double *level, int32_t *has_value);

/* ---- the TTL trigger track: detections as the pulses the rig emits ----
 * The reference's product is a TTL pulse on an audio output, recorded beside the microphone:
 *   Processor.swift:128-148          a callback buffer is `seen` if any evaluation it made available has lastDetected
 *   ProcessorAudio :217-221          prepareOutputFor then calls createHighOutput(channel, forDuration: 0.001)
 *   AudioInterface.swift:442-445     outputHighFor[channel] = Int(duration * rate) -- set, not added to (:444)
 *   AudioInterface.swift:13-40       renderOutput writes 1.0 for that many samples from the next render buffer on
 *   ProcessorArduino :266-291        the same monostable counted in callbacks: high until 20 callbacks without a syllable
 * With D = first_index, hop, callback buffers of L = buffer_length samples (a power of two, 8 <= L <= 4096; the reference's 32),
 * pulse width N = width_samples >= 1 and output latency Lat = latency_samples >= 0 (the reference's README: "up to 5 ms"; 0 is the
 * model's default):
 *   b(e)     = (D + e hop - 1) / L     the buffer whose callback makes evaluation e available (integer division); the same
 *                                      statement as syldet_levels_eval_range(..., buffers_per_reading = 1, ...)
 *   seen(b)  = some e < n_evals with b(e) = b has flags[c][e] != 0
 *   t_b      = (b + 1) L + Lat         a seen buffer arms the output as its callback returns: the next render buffer's first sample
 *   track[c][s] = 1 iff some seen buffer b has t_b <= s < t_b + N      (0 <= s < n_samples; else 0)
 * A later arm inside a pulse extends it to its own t_b + N (:444 sets), which is the union above.
 * An onset is a seen buffer b with no seen buffer in [b - N / L, b) (integer division; pulses that abut are one pulse); its
 * sample is t_b; onsets at t_b >= n_samples are not reported.  The onsets are the rising edges of the track.
 * The Arduino form is N = 20 L.  syldet_trigger_width(seconds, rate) is Int(seconds * rate) (:444); -1 for a result below 1 or
 * not finite.
 * d_flags [C][n_evals] as syldet_run_device* wrote them: the reference's lastDetected is output 0 against its threshold
 * (SyllableDetector.swift:27-31), which is SYLDET_RULE_FIRST; flags of another rule give that rule's pulses.  D and hop come from
 * the handle as in syldet_trace*; plain, multi-network and mixed banks alike.
 *   d_track  [C][track_stride], the first n_samples of each row: fp32 1.0f / 0.0f (the reference's floats), int16 32767 / 0 (the
 *            trace's convention)
 *   d_frames [n_samples][C] int16 (syldet_trigger_interleaved_device_s16), or [n_samples][2 C] (syldet_trigger_mux_device_s16):
 *            frame f = (audio[0][f], ttl[0][f], audio[1][f], ttl[1][f], ...), the audio copied bit for bit from the planar int16
 *            rows syldet_run_device_s16 takes -- the stereo file a DAQ would have recorded, for every channel at once
 *   d_indices [C][capacity] int64, d_counts [C] int64: the onsets' samples in order, and how many there are (the convention of
 *            syldet_detections_device: the first min(count, capacity) are written)
 * Every call scans the flags into a table last_seen[c][b] (the greatest seen buffer <= b, or -1; B' = ceil((n_samples + L - 1) / L)
 * entries a channel, scratch the handle keeps and grows) and then expands or compacts from it: syldet_timings lists
 * "trigger_scan_kernel" and one of "trigger_kernel", "trigger_interleaved_s16_kernel", "trigger_onsets_kernel".
 * Statuses, before any device is touched: SYLDET_ERR_INVALID_ARGUMENT for a NULL handle or pointer, negative counts, a stride
 * below n_samples, an L that is not a power of two in [8, 4096], N < 1 or N > 2^24, Lat < 0 or Lat > 2^24.  n_samples == 0
 * writes no sample (the onsets' counts are 0); n_evals == 0 writes zeros.  The device forms follow the handle's rule of one
 * stream at a time.                                                                                                          */
int64_t syldet_trigger_width(double seconds, double rate);
int syldet_trigger_device(syldet_t *h, const uint8_t *d_flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                          int64_t latency_samples, float *d_track, int64_t n_samples, int64_t track_stride, void *hip_stream);
int syldet_trigger_device_s16(syldet_t *h, const uint8_t *d_flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                              int64_t latency_samples, int16_t *d_track, int64_t n_samples, int64_t track_stride, void *hip_stream);
int syldet_trigger_interleaved_device_s16(syldet_t *h, const uint8_t *d_flags, int64_t n_evals, int32_t buffer_length,
                                          int64_t width_samples, int64_t latency_samples, int16_t *d_frames, int64_t n_samples,
                                          void *hip_stream);
int syldet_trigger_mux_device_s16(syldet_t *h, const uint8_t *d_flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                                  int64_t latency_samples, const int16_t *d_samples, int64_t channel_stride, int16_t *d_frames,
                                  int64_t n_samples, void *hip_stream);
int syldet_trigger_onsets_device(syldet_t *h, const uint8_t *d_flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                                 int64_t latency_samples, int64_t n_samples, int64_t *d_indices, int64_t capacity, int64_t *d_counts,
                                 void *hip_stream);
/* the track and its onsets from ONE scan of the flags (what a rehearsal of a recording wants: syldet_timings lists
 * "trigger_scan_kernel", "trigger_kernel", "trigger_onsets_kernel"); the results are those of the two calls above                  */
int syldet_trigger_rehearse_device(syldet_t *h, const uint8_t *d_flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                                   int64_t latency_samples, float *d_track, int64_t n_samples, int64_t track_stride,
                                   int64_t *d_indices, int64_t capacity, int64_t *d_counts, void *hip_stream);
int syldet_trigger_rehearse_device_s16(syldet_t *h, const uint8_t *d_flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                                       int64_t latency_samples, int16_t *d_track, int64_t n_samples, int64_t track_stride,
                                       int64_t *d_indices, int64_t capacity, int64_t *d_counts, void *hip_stream);
/* host pointers, blocking (as syldet_trace is to syldet_trace_device) */
int syldet_trigger(syldet_t *h, const uint8_t *flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                   int64_t latency_samples, float *track, int64_t n_samples, int64_t track_stride);
int syldet_trigger_s16(syldet_t *h, const uint8_t *flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                       int64_t latency_samples, int16_t *track, int64_t n_samples, int64_t track_stride);
int syldet_trigger_onsets(syldet_t *h, const uint8_t *flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                          int64_t latency_samples, int64_t n_samples, int64_t *indices, int64_t capacity, int64_t *counts);
/* Streaming, host only: the two reference functions.  syldet_trigger_arm is createHighOutput (the channel's counter = width_samples,
 * >= 0); syldet_trigger_render is renderOutput for one channel: out[i] = i < high ? 1 : 0 for n_frames frames, and the counter
 * goes down by min(high, n_frames).  The counter is an atomic: an audio-output thread may render beside the consumer that arms
 * (an arm that lands inside a render is kept whole).  A handle that never arms renders zeros and does what it always did.    */
int syldet_trigger_arm(syldet_t *h, int32_t channel, int64_t width_samples);
int syldet_trigger_render(syldet_t *h, int32_t channel, float *out, int32_t n_frames);

/* ---- measurement (replaces the reference's Time stopwatch, SyllableDetector/Time.swift:36-100,
 * which wraps processNewValue in ViewControllerSimulator.swift:309-319) ----
 * With profiling enabled every kernel of a batch call is bracketed by HIP events on the stream it
 * is launched on.  syldet_last_timings blocks until the last call's events have completed and
 * returns up to `capacity` kernel durations in milliseconds, in launch order, with their names.
 * The exact recomputation behind the fused kernels' precision guard ("fixup_kernel") is listed for
 * the calls that gave it work (syldet_fixup_stats' items > 0): on ordinary audio it is an empty launch.
 * Its duration is the kernel's own (device clock, first workgroup in to last out), and reading it
 * waits for the stream the call was made on.                                                       */
int syldet_profile(syldet_t *h, int enable);
int syldet_last_timings(syldet_t *h, double *milliseconds, const char **names, int32_t capacity, int32_t *count);
/* Keep the events of the last `calls` batch calls instead of one (waits for the handle's stream, drops what was recorded), so
 * that a measurement loop need not wait for every call before making the next; syldet_timings reads the call made
 * `calls_back` calls before the last one (0: the last), *count = 0 if that call is not held.                              */
int syldet_profile_history(syldet_t *h, int32_t calls);
int syldet_timings(syldet_t *h, int32_t calls_back, double *milliseconds, const char **names, int32_t capacity, int32_t *count);
/* The fused kernels compute on a block-floating-point grid.  The symmetric-fold kernel (the reference's example class: at
 * most 4 hidden units, no normaliser or l2normalize, windows of 64 / 128 / 192 / 256 samples) gives every FRAME its own
 * power-of-two scale: its results are a function of the samples under the window alone -- the same bits whether the audio
 * arrives through the streaming calls or a batch call, however it is tiled -- and only what no grid can hold (an infinite
 * sample, levels 2^45 apart inside one window) is recomputed.  The two older kernels (wider networks, normalize /
 * normalizestd chains) scale per 64 / 128-frame pass: evaluations whose windows that grid cannot hold to the 1e-5 contract --
 * a quiet stretch right behind a click, a level step of hundreds of dB -- are detected on the device and recomputed from
 * the samples in fp64 (and NaN, which the reference yields exactly for the windows that contain the offending sample:
 * NeuralNet.swift:47-59, appears exactly there); between two tilings of the same audio their results agree to a few 1e-7.  *items = 16-evaluation work items the last completed batch call of this handle recomputed
 * (0 for ordinary audio), *overflow = 1 if a work list was ever too small (never, by construction).  Blocks; call it after
 * the stream the batch call ran on has been synchronised.  No reference counterpart (diagnostic).                       */
int syldet_fixup_stats(syldet_t *h, int64_t *items, int32_t *overflow);
/* How the batch call tiles a channel for n_samples per channel: evaluations per workgroup segment of the fused kernels
 * (consecutive segments of a channel are computed by different workgroups; 0: the engine in use has no such seams).
 * Results do not depend on it; verification uses it to aim spot checks at the seams.  No reference counterpart.          */
int64_t syldet_segment_evals(const syldet_t *h, int64_t n_samples);
/* Which instantiation of the fused kernels ran: *kernel = 0 the 8-wave kernel, 1 the register-resident-basis kernel, 2 the
 * symmetric-fold kernel; params = that instantiation's template arguments in declaration order (booleans as 0 / 1, defaulted
 * ones included, zeros behind the last) -- of the calling thread's most recent batch or spectrogram call through this handle.
 * SYLDET_ERR_UNSUPPORTED if that call ran no fused kernel (or the thread made none through this handle);
 * SYLDET_ERR_INVALID_ARGUMENT for a NULL pointer.  Verification names the compiled form a case reached with it; results do not
 * depend on it.  No reference counterpart (diagnostic).                                                                   */
int syldet_last_fused_form(const syldet_t *h, int32_t *kernel, int32_t params[10]);
/* The same answer from the host alone, without a device: the instantiation a handle of these configurations would run for a
 * batch of n_samples per channel over n_channels channels.  n_nets == 1 and channel_net NULL: the handle syldet_create makes
 * of cfgs[0]; otherwise syldet_create_multi's.  s16 != 0: the batch is 16-bit PCM in rows of whole words (syldet_run_device_s16
 * on an aligned base with an even stride).  spectrogram != 0: syldet_spectrogram_device's transform instead of the batch call.
 * The plan is built as the create call builds it, under the same SYLDET_FUSED_* switches, and handed to the very launchers the
 * batch call uses, which record the form and return before they touch the device.  SYLDET_ERR_UNSUPPORTED (syldet_last_error
 * says why) for what is not on the fused engine: what AUTO keeps elsewhere, batches without an evaluation; the create calls'
 * statuses for what they refuse.  No reference counterpart (diagnostic).                                                */
int syldet_fused_form_of_config(const syldet_config_t *const *cfgs, int32_t n_nets, const int32_t *channel_net, int32_t n_channels,
                                int64_t n_samples, int32_t s16, int32_t spectrogram, int32_t engine, int32_t *kernel, int32_t params[10]);
/* 1 while the calling thread is inside syldet_fused_form_of_config's dry run of the launchers, 0 at any other time -- a failed
 * plan included (verification: a launch after it must reach the device).                                                    */
int32_t syldet_fused_dry_run_active(void);

/* ---- streaming: the reference's per-detector API, one call per channel ----
 * Each channel owns a single-producer / single-consumer sample ring like the reference's
 * TPCircularBuffer (TPCircularBuffer.h:14,102-189): append* never locks or allocates and may run
 * on an audio I/O thread (AudioInterface.swift:67-70 -> Processor.swift:124) while another thread
 * processes.  appendAudioData(_:withSamples:), SyllableDetector.swift:129-132              */
int syldet_append(syldet_t *h, int32_t channel, const float *data, int64_t n_samples);
/* appendInterleavedData(_:withSamples:fromChannel:ofTotalChannels:),
 * CircularShortTimeFourierTransform.swift:203-217: de-interleaves frame-major audio into
 * every channel of the bank (total_channels == syldet_channels(h))                       */
int syldet_append_interleaved(syldet_t *h, const float *data, int64_t n_frames, int32_t total_channels);
/* The same call's fromChannel: the bank sits on a SUBSET of a wider device stream -- channel c of the bank takes channel
 * source_channel[c] of the total_channels interleaved in `data` (appendInterleavedData(_:withSamples:fromChannel:ofTotalChannels:),
 * CircularShortTimeFourierTransform.swift:203-217, takes one channel of the stream per call: :213's stride is the stream's width).
 * source_channel: syldet_channels(h) entries, each in [0, total_channels); a stream channel may feed several bank channels.    */
int syldet_append_interleaved_channels(syldet_t *h, const float *data, int64_t n_frames, int32_t total_channels,
                                       const int32_t *source_channel);
/* syldet_append / syldet_append_interleaved for 16-bit PCM: sample x goes into the fp32 ring as x * 2^-15 (exact), with the
 * same checks and the same ring-full rule (the ring's room is counted in fp32 samples): every later result is the fp32
 * appends' bit for bit.                                                                                                    */
int syldet_append_s16(syldet_t *h, int32_t channel, const int16_t *data, int64_t n_samples);
int syldet_append_interleaved_s16(syldet_t *h, const int16_t *data, int64_t n_frames, int32_t total_channels);
/* processNewValue() -> Bool, SyllableDetector.swift:153-217: 1 = a new evaluation is in
 * last_outputs, 0 = not enough data yet                                                  */
int syldet_process_new_value(syldet_t *h, int32_t channel);
/* The consumer loop of a multi-channel Processor (`for d in detectors { while d.processNewValue() … }`,
 * Processor.swift:128-141) in one device round trip: evaluates everything every channel has pending
 * (one staged copy + one launch per distinct evaluation count, i.e. one when the channels are fed
 * together) and queues the results; the following syldet_process_new_value calls hand them out one by
 * one without touching the device.  *n_queued (optional) = evaluations added over all channels.      */
int syldet_process_all(syldet_t *h, int64_t *n_queued);
/* evaluations computed and not yet handed out by syldet_process_new_value                */
int64_t syldet_pending_evaluations(const syldet_t *h, int32_t channel);
/* lastOutputs, :26 (zeros before the first evaluation, :70)                              */
int syldet_last_outputs(const syldet_t *h, int32_t channel, float *out);
/* lastDetected, :27-31                                                                   */
int syldet_last_detected(const syldet_t *h, int32_t channel);
/* seenSyllable(), :220-230: drains every pending evaluation, 1 if any was detected       */
int syldet_seen_syllable(syldet_t *h, int32_t channel);

/* ---- ingest: the steps immediately before the path ----
 * Frame-major (interleaved) audio, as a decoder or a multi-channel device delivers it:
 * appendInterleavedData(_:withSamples:fromChannel:ofTotalChannels:),
 * CircularShortTimeFourierTransform.swift:203-217, for every channel at once.
 * interleaved [n_frames][total_channels] fp32 -> rows of channels first_channel ..
 * first_channel + n_channels - 1 in out [n_channels][out_stride].                        */
int syldet_deinterleave_device(const float *d_interleaved, int64_t n_frames, int32_t total_channels,
                               int32_t first_channel, int32_t n_channels, float *d_out, int64_t out_stride,
                               void *hip_stream);
/* the same for 16-bit PCM frames: channels 0 .. n_channels - 1 of total_channels -> int16 rows [n_channels][out_stride] (the
 * rows syldet_run_device_s16 and syldet_trigger_mux_device_s16 take)                                                        */
int syldet_deinterleave_device_s16(const int16_t *d_interleaved, int64_t n_frames, int32_t total_channels, int32_t n_channels,
                                   int16_t *d_out, int64_t out_stride, void *hip_stream);
/* The batch call on interleaved audio (total_channels == syldet_channels(h)): de-interleave
 * on the device, then exactly syldet_run_device / syldet_run.                             */
int syldet_run_interleaved_device(syldet_t *h, const float *d_interleaved, int64_t n_frames, int32_t total_channels,
                                  float *d_outputs, uint8_t *d_flags, void *hip_stream);
int syldet_run_interleaved(syldet_t *h, const float *interleaved, int64_t n_frames, int32_t total_channels,
                           float *outputs, uint8_t *flags);
/* ... on 16-bit PCM frames [n_frames][total_channels] int16 (x meaning float(x) * 2^-15): de-interleaved on the device into
 * int16 rows (2 bytes a sample), then exactly syldet_run_device_s16; the host form copies int16.  Bit-identical to the fp32
 * twin fed float(x) * 2^-15, with its checks and statuses, made before any device is touched.                               */
int syldet_run_interleaved_device_s16(syldet_t *h, const int16_t *d_interleaved, int64_t n_frames, int32_t total_channels,
                                      float *d_outputs, uint8_t *d_flags, void *hip_stream);
int syldet_run_interleaved_s16(syldet_t *h, const int16_t *interleaved, int64_t n_frames, int32_t total_channels,
                               float *outputs, uint8_t *flags);

/* ---- the exchange step of the multi-GPU path (no reference counterpart: the reference runs one process) ----
 * Channels shard across GPUs with no data-path collective; the one exchange is the gather of the detection
 * flags, and it travels as bits: bit b of byte t of a row = flag 8 t + b, rows padded to whole bytes
 * ((row_len + 7) / 8 bytes per row).  Device pointers (d_flags of the unpack 8-byte aligned), asynchronous on
 * `hip_stream`; rows <= 65535.                                                                            */
int syldet_pack_flags_device(const uint8_t *d_flags, int64_t rows, int64_t row_len, uint8_t *d_bits, void *hip_stream);
int syldet_unpack_flags_device(const uint8_t *d_bits, int64_t rows, int64_t row_len, uint8_t *d_flags, void *hip_stream);

/* ---- one bank over several GPUs, ONE process ----
 * The reference is one process that owns every channel: Processor.swift:57-59 builds one SyllableDetector per channel and
 * one serial queue drains them all (:82, :128-141); main.swift:86-89 builds one TrackDetector per track and one loop runs
 * them (:126-130).  A sharded bank keeps that shape for a host with several MI355X: one handle, one call per batch; the
 * library places a sub-bank and a stream on every listed device, splits the channels into contiguous blocks (the first
 * n_channels % n_devices devices take one more), and -- with fewer channels than devices -- splits a channel's TIME axis
 * instead: a shard then computes a contiguous range of one channel's evaluations from its samples plus a halo of
 * (timeRange - 1) hop + window - hop (+ gap) samples (evaluation e is frames e .. e + timeRange - 1, frame j is samples
 * [j hop + gap, j hop + gap + window): SyllableDetector.swift:153-217, CircularShortTimeFourierTransform.swift:286-302).
 * The kernels AUTO selects for the benchmark configurations scale per frame (fold kernel) or per hop-aligned block
 * (block-transform, FFT kernels), so a shard's results there are the unsharded bank's bit for bit; the pass-scaled fused
 * kernels (SYLDET_FUSED_NOFOLD / _CLASSIC, shapes outside the fold kernel's class) agree between tilings to a few 1e-7 only.
 * The data path has no collective.  The one exchange -- every device receives every channel's detection flags -- is ONE
 * all-gather of the bit-packed rows per batch, on RCCL communicators the library makes itself (ncclCommInitAll, one
 * process; librccl is loaded on first use, so hosts with one GPU never pay for it).                                   */
typedef struct syldet_sharded syldet_sharded_t;

typedef struct {
    int32_t device;              /* HIP device of the shard                                                */
    int32_t first_channel;       /* the shard owns channels [first_channel, first_channel + channels)      */
    int32_t channels;
    int32_t part, parts;         /* its place along the time axis of its channel (0 of 1 unless n_channels < n_devices) */
} syldet_shard_t;

/* how the flags travel between the devices of a sharded bank */
typedef enum {
    SYLDET_EXCHANGE_RCCL = 0,        /* one ncclAllGather per device inside one ncclGroupStart/End (xGMI)            */
    SYLDET_EXCHANGE_PEER_COPY = 1    /* hipMemcpyPeerAsync of every shard's packed rows to every device: no RCCL in
                                        the process; also what a bank with one device listed twice uses (a rehearsal
                                        of the shard logic on a one-GPU box: RCCL refuses duplicate devices)        */
} syldet_exchange_t;

/* The shard table alone (host arithmetic, no device): out[i] for i < n_shards, device = i. */
int syldet_shard_table(int32_t n_channels, int32_t n_shards, syldet_shard_t *out);
/* Evaluations [*first, *first + *count) of a channel with n_evals evaluations that part `part` of `parts` computes, and the
 * samples [*s0, *s1) of the recording it reads for them (cfg gives hop, gap, window, timeRange).                         */
int syldet_shard_evaluations(int64_t n_evals, int32_t parts, int32_t part, int64_t *first, int64_t *count);
int syldet_shard_samples(const syldet_config_t *cfg, int64_t first_eval, int64_t count, int64_t *s0, int64_t *s1);

int syldet_create_sharded(const syldet_config_t *cfg, int32_t n_channels, const int32_t *devices, int32_t n_devices,
                          int32_t engine, int32_t exchange, syldet_sharded_t **out);
int syldet_sharded_destroy(syldet_sharded_t *b);
int32_t syldet_sharded_channels(const syldet_sharded_t *b);
int32_t syldet_sharded_shards(const syldet_sharded_t *b);
int syldet_sharded_shard(const syldet_sharded_t *b, int32_t shard, syldet_shard_t *out);
/* the shard's own bank (borrowed: destroyed with the sharded bank), the stream its kernels (and own results) are queued on,
 * and the stream its share of the exchange runs on (d_flags_all[shard] is complete when THAT stream has drained: the exchange
 * of batch i runs beside the kernels of batch i + 1, as Processor.swift:128-141's queue hands out results while audio arrives) */
syldet_t *syldet_sharded_bank(syldet_sharded_t *b, int32_t shard);
void *syldet_sharded_stream(syldet_sharded_t *b, int32_t shard);
void *syldet_sharded_exchange_stream(syldet_sharded_t *b, int32_t shard);
/* For a recording of n_samples per channel: the samples [*s0, *s1) shard `shard` reads of each of its channels (all of them
 * unless time-sharded) and the evaluations [*e0, *e0 + *count) it computes.  Any output pointer may be NULL.            */
int syldet_sharded_ranges(const syldet_sharded_t *b, int32_t shard, int64_t n_samples, int64_t *s0, int64_t *s1,
                          int64_t *e0, int64_t *count);
/* Host buffers, the whole bank in one call: samples [C][channel_stride] -> outputs [C][E][outputs], flags [C][E], as
 * syldet_run.  Every shard's copies and kernels are queued before any is waited for (one pipelined H2D / kernel / D2H
 * chain per device); results land in the caller's rows directly, so this form needs no collective.  Blocks.              */
int syldet_sharded_run(syldet_sharded_t *b, const float *samples, int64_t n_samples, int64_t channel_stride,
                       float *outputs, uint8_t *flags);
/* Device buffers: d_samples[i] is shard i's block on its device -- [channels_i][strides[i]] rows holding the shard's
 * sample range (syldet_sharded_ranges) of a recording of n_samples per channel; d_outputs[i] [channels_i][count_i][outputs]
 * and d_flags[i] [channels_i][count_i] receive its own results (either array, or any entry, may be NULL);
 * d_flags_all[i], when the array is given, receives EVERY channel's flags [C][E] on device i (8-byte aligned) through the
 * one exchange.  The bank's streams are its own (hipStreamNonBlocking): work the caller has queued elsewhere that produces the
 * samples -- or still reads memory now handed over as a result array -- must have finished (or be ordered by the caller's own
 * events on syldet_sharded_stream) before the call.  Asynchronous: every shard's kernel is launched before the exchange is queued, and the exchange runs on
 * streams of its own (two sets of buffers in turn), so the next call's kernels start without waiting for this call's
 * collective.  The queueing itself runs on the bank's launcher threads, every shard at once (syldet_sharded_launcher_threads);
 * the call returns when every shard's work is queued.  Results are complete after syldet_sharded_synchronize (or after synchronising syldet_sharded_stream(b, i) for
 * shard i's own results, syldet_sharded_exchange_stream(b, i) for d_flags_all[i]).                                       */
int syldet_sharded_run_device(syldet_sharded_t *b, const float *const *d_samples, int64_t n_samples, const int64_t *strides,
                              float *const *d_outputs, uint8_t *const *d_flags, uint8_t *const *d_flags_all);
int syldet_sharded_synchronize(syldet_sharded_t *b);
/* RCCL ranks behind the exchange (0 under SYLDET_EXCHANGE_PEER_COPY) */
int32_t syldet_sharded_rccl_ranks(const syldet_sharded_t *b);
/* Brings the exchange up NOW instead of inside the first gathering batch: under SYLDET_EXCHANGE_RCCL loads librccl and makes
 * the communicators (ncclCommInitAll over the bank's devices); under the copy exchange enables peer access between the bank's
 * devices where the hardware offers it.  A caller that wants to fall back (a host whose RCCL does not come up) calls this
 * right after syldet_create_sharded and, on an error, destroys the bank and makes it again with SYLDET_EXCHANGE_PEER_COPY
 * -- in the same process: nothing here needs a fresh one.                                                                   */
int syldet_sharded_connect(syldet_sharded_t *b);
/* Launcher threads of the bank: one per shard, alive as long as the bank, each with its shard's device current; a batch call's
 * per-shard queueing (kernel, packing, the exchange's waits and records, unpacking) runs on all of them at once.  0 for a bank
 * of one shard and for banks made under SYLDET_SHARDED_INLINE=1, whose calls queue shard after shard on the caller's thread
 * (the reference's own shape: one serial queue, Processor.swift:82).                                                         */
int32_t syldet_sharded_launcher_threads(const syldet_sharded_t *b);

/* ResamplerLinear, Common/Resampler.swift:20-76 (used when the device rate differs from the
 * network's: Processor.swift:116-121, ViewControllerProcessor.swift:247-250), for n_channels
 * independent streams fed in lock-step.  Stateful like the reference: the fractional
 * position (`offset`) and the last input sample of every channel carry over to the next
 * call.  Results are bit-identical to the reference's arithmetic order (fp32, no FMA).    */
typedef struct syldet_resampler syldet_resampler_t;
int syldet_resampler_create(double rate_in, double rate_out, int32_t n_channels, int32_t device,
                            syldet_resampler_t **out);
int syldet_resampler_destroy(syldet_resampler_t *r);
/* samples per channel the next call produces from n_in input samples (:40)               */
int64_t syldet_resampler_count(const syldet_resampler_t *r, int64_t n_in);
/* resampleVector(_:ofLength:), :36-69.  in [C][in_stride] -> out [C][out_stride]; *n_out
 * (host) receives the per-channel output length (= syldet_resampler_count before the call) */
int syldet_resample_device(syldet_resampler_t *r, const float *d_in, int64_t n_in, int64_t in_stride, float *d_out,
                           int64_t out_stride, int64_t *n_out, void *hip_stream);
int syldet_resample(syldet_resampler_t *r, const float *in, int64_t n_in, int64_t in_stride, float *out,
                    int64_t out_stride, int64_t *n_out);

/* Whole-recording rate conversion for offline input.  The reference's command line tool never resamples itself: it asks
 * AVFoundation to deliver every track at the network's rate (audioSettings, SyllableDetector.swift:19-23, handed to
 * AVAssetReaderTrackOutput at TrackDetector.swift:35).  This is that step for a decoded file: output sample i is the linear
 * interpolation of the input at position i * rate_in / rate_out, the position computed in fp64 (ResamplerLinear above is a
 * streaming object for short live buffers: its fp32 position ramp and its buffer carry are not meant for minutes of audio
 * in one call).  Stateless.  in [C][in_stride] -> out [C][out_stride]; *n_out = syldet_convert_rate_count(n_in, ...).    */
int64_t syldet_convert_rate_count(int64_t n_in, double rate_in, double rate_out);
int syldet_convert_rate_device(const float *d_in, int64_t n_in, int64_t in_stride, int32_t n_channels, double rate_in,
                               double rate_out, float *d_out, int64_t out_stride, int64_t *n_out, void *hip_stream);

/* The same step band-limited: what AVFoundation's delivery at the network's rate (audioSettings, SyllableDetector.swift:19-23,
 * TrackDetector.swift:35) is and the linear form above is not -- linear interpolation does not filter before it decimates (48 ->
 * 44.1 kHz folds 22.05-24 kHz back into the band) and droops the band by sinc^2(f / rate_in).  AVFoundation's converter is not
 * specified; this library's convention is a Kaiser-windowed sinc evaluated at exact fp64 positions, zeros beyond both ends:
 *     Z   zero_crossings, the half width in zero crossings   4 <= Z <= 64       default 32
 *     b   beta, the Kaiser window's                          0 <= b <= 20       default 12.0 (about 117 dB of stop band)
 *     r   rolloff                                            0 <  r <= 1        default 0.9
 *     s      = min(1, rate_out / rate_in) * r         the cutoff as a fraction of the input's Nyquist frequency
 *     H      = Z / s                                  the half width in input samples
 *     p_i    = i * rate_in / rate_out                 fp64, i = 0 .. n_out - 1, n_out = syldet_convert_rate_count(n_in, ...)
 *     h(t)   = s * sinc(s t) * I0(b sqrt(1 - (t / H)^2)) / I0(b)  for |t| < H, else 0;  sinc(x) = sin(pi x) / (pi x)
 *     out[i] = sum over k = ceil(p_i - H) .. floor(p_i + H) of x[k] * h(p_i - k),   x[k] = 0 for k outside [0, n_in)
 * No renormalisation at DC: the gain error is the design's own ripple, at the level of the stop band.  The output length is the
 * linear form's, so nothing behind the converter changes shape.  rate_in == rate_out is a low-pass at r of Nyquist, not a copy.
 * At the default Z the transition band is about 0.12 of the sampling rate wide and centred on the cutoff; with r = 0.9 the stop
 * band begins about 1 % above the new Nyquist frequency.
 *
 * syldet_sinc_defaults writes the defaults (NULL: skipped).  syldet_sinc_coefficient is h(t) in fp64, NaN for parameters the
 * device calls refuse; syldet_sinc_taps is 2 floor(H) + 1, the number of taps of an output that falls on an input sample (an
 * output between two samples may read one more: floor(2 H) + 1 at most), or -1 for such parameters.  These three are host
 * functions and need no device.                                                                                              */
void syldet_sinc_defaults(int32_t *zero_crossings, double *beta, double *rolloff);
double syldet_sinc_coefficient(double t, double rate_in, double rate_out, int32_t zero_crossings, double beta, double rolloff);
int64_t syldet_sinc_taps(double rate_in, double rate_out, int32_t zero_crossings, double rolloff);
/* in [C][in_stride] -> out [C][out_stride] fp32, asynchronous on the stream, on the current device; *n_out (host, may be NULL) =
 * syldet_convert_rate_count(n_in, ...).  The _s16 form takes the rows syldet_deinterleave_device_s16 writes, x meaning
 * float(x) * 2^-15, and gives the bits of the fp32 form fed those floats.  Stateless: an output depends on its own row, its
 * index and the parameters alone -- the channel count and the strides do not change its bits, nor does the run.  The device
 * evaluates h through an fp32 table of the unit filter sinc(tau) * kaiser(tau / Z) (at least 512 entries a zero crossing,
 * interpolated linearly, the sum in fp32 in the order of k): for every output |out - exact| <= T 2^-24 A + 2^-21 X with T the
 * number of k in the sum above, A = sum |h x| and X = sum |x|.  The bound as a whole is the contract, not its terms: a
 * coefficient next to the centre may be up to 1.6e-6 from the exact one, the others far closer than 2^-21.  That table, 64 KiB (Z <= 32) or 128 KiB, sits on the device in
 * a cache keyed by (Z, beta) and the device: the first call for a parameter set on a device builds it on the host and makes a
 * blocking copy, as syldet_trace* does for its threshold table; later calls only queue the kernel.  The cache keeps 16 tables
 * and gives up the oldest for a new one (which waits for the device).  These calls take no handle, so syldet_timings does not
 * list their kernel (convert_rate_sinc_kernel); time it with events on the stream.
 * Statuses, before any device is touched: SYLDET_ERR_INVALID_ARGUMENT for a NULL buffer, n_in < 0, n_channels outside
 * [1, 65535], a rate that is not positive, Z, beta or rolloff outside the ranges above and (n_channels > 1) a stride below its
 * row; SYLDET_ERR_UNSUPPORTED for rate_in / rate_out outside [1/16, 16], which bounds the inputs a workgroup stages, and for
 * H > 65536 (a rolloff below 1/64 at the widest filter and ratio): an output costs 2 H taps, and the limit bounds a launch's
 * run time.  n_in == 0 writes nothing and sets *n_out = 0.            */
int syldet_convert_rate_sinc_device(const float *d_in, int64_t n_in, int64_t in_stride, int32_t n_channels, double rate_in,
                                    double rate_out, int32_t zero_crossings, double beta, double rolloff, float *d_out,
                                    int64_t out_stride, int64_t *n_out, void *hip_stream);
int syldet_convert_rate_sinc_device_s16(const int16_t *d_in, int64_t n_in, int64_t in_stride, int32_t n_channels, double rate_in,
                                        double rate_out, int32_t zero_crossings, double beta, double rolloff, float *d_out,
                                        int64_t out_stride, int64_t *n_out, void *hip_stream);

/* The band-limited converter as a stream: ResamplerSinc, a second conformer of the reference's Resampler protocol
 * (Common/Resampler.swift:12-15; Processor.swift:115-120 puts one in front of appendAudioData when the device's rate is not the
 * network's).  The contract has no tolerance: however a recording is cut into pushes, the concatenated outputs of the pushes
 * and the flush are syldet_convert_rate_sinc_device's on the whole rows, bit for bit.  Everything is the convention above; only
 * the emission rule is new:
 *     N          input samples received so far (per channel), M outputs emitted so far
 *     p_i        = (double)i * rate_in / rate_out, i absolute (counted from the stream's first output); H, s, the taps and the
 *                order of the sum are those of syldet_convert_rate_sinc_device
 *     ready      output i is emitted as soon as floor(p_i + H) <= N - 1: every tap it will ever have is present, so the whole-
 *                recording form's cut at the row's end is not active and its bits cannot depend on what comes later.  The
 *                predicate is evaluated in fp64 in the kernel's order of operations and is monotone in i; ready(N) is the number of
 *                outputs that satisfy it, and after every push M = ready(N) <= syldet_convert_rate_count(N, ...).
 *     flush      ends the recording at N samples: emits i = M .. syldet_convert_rate_count(N, ...) - 1 with their taps cut at
 *                N - 1, as the whole-recording call does at a row's end.  The stream is then finished: a push is refused
 *                (SYLDET_ERR_INVALID_ARGUMENT) until syldet_sinc_resampler_reset; another flush emits nothing.
 *     history    the next output reads inputs from max(ceil(p_M - H), 0) on, never more than ceil(2 H) + 2 samples behind N; the
 *                handle keeps that many per channel on the device as fp32 (two buffers, used in turn).  An int16 push is widened
 *                as it is kept (x * 2^-15, exact), so fp32 and int16 pushes may alternate on one handle.
 *     latency    outputs trail inputs by H input samples: 35.6 (0.74 ms) at 48 -> 44.1 kHz with the defaults, 8.9 at Z = 8.
 * syldet_sinc_ready is ready(n_in_total) in host arithmetic, no device; -1 for parameters the device calls refuse.
 *
 * syldet_sinc_resampler_create checks its arguments as syldet_convert_rate_sinc_device does (same ranges, same statuses; then
 * SYLDET_ERR_NO_DEVICE), builds the handle's OWN copy of the filter's table (the same floats as the stateless calls' cache, which
 * gives up its oldest table and so cannot lend one) and the history, and blocks.  reset: N = M = 0, not finished.  position
 * reads N, M and whether the stream is finished (any pointer may be NULL).  count: the outputs a push of n_in samples would emit
 * now; flush_count: those a flush would.
 *
 * The device calls: in [C][in_stride] (fp32, or int16 meaning x * 2^-15) -> out [C][out_stride] fp32, *n_out (host, may be NULL)
 * the outputs per channel this call emitted, which is syldet_sinc_resampler_count taken before it.  N and M are host arithmetic:
 * a device push never synchronises, never allocates and never copies from the host; it queues at most two kernels
 * (convert_rate_sinc_stream_kernel when it emits, sinc_carry_kernel for the history).  ALL device work of one handle must be on
 * one stream, or ordered by the caller: a push reads the history the push before it wrote.  The pushed rows must stay valid until
 * that work has run.  Statuses, decided before any device is touched and before any state changes -- a refused call leaves N, M
 * and the history as they were, and a correct call after it gives the right bits: SYLDET_ERR_INVALID_ARGUMENT for a NULL handle,
 * n_in < 0, a push on a finished stream, a NULL input with n_in > 0, a NULL output when the call emits something (d_out may be
 * NULL only when it emits nothing) and, with more than one channel, a stride below its row (in_stride < n_in, out_stride < the
 * count).  n_in == 0 is legal and emits nothing.
 *
 * syldet_sinc_resample and syldet_sinc_resampler_flush take host buffers and block (resampleArray's shape, as syldet_resample
 * is for the linear one), on a stream of the handle's own.                                                                  */
typedef struct syldet_sinc_resampler syldet_sinc_resampler_t;
int64_t syldet_sinc_ready(int64_t n_in_total, double rate_in, double rate_out, int32_t zero_crossings, double rolloff);
int syldet_sinc_resampler_create(double rate_in, double rate_out, int32_t n_channels, int32_t device, int32_t zero_crossings,
                                 double beta, double rolloff, syldet_sinc_resampler_t **out);
int syldet_sinc_resampler_destroy(syldet_sinc_resampler_t *r);
int syldet_sinc_resampler_reset(syldet_sinc_resampler_t *r);
int syldet_sinc_resampler_position(const syldet_sinc_resampler_t *r, int64_t *n_in_total, int64_t *n_out_total, int32_t *finished);
int64_t syldet_sinc_resampler_count(const syldet_sinc_resampler_t *r, int64_t n_in);
int64_t syldet_sinc_resampler_flush_count(const syldet_sinc_resampler_t *r);
int syldet_sinc_resample_device(syldet_sinc_resampler_t *r, const float *d_in, int64_t n_in, int64_t in_stride, float *d_out,
                                int64_t out_stride, int64_t *n_out, void *hip_stream);
int syldet_sinc_resample_device_s16(syldet_sinc_resampler_t *r, const int16_t *d_in, int64_t n_in, int64_t in_stride, float *d_out,
                                    int64_t out_stride, int64_t *n_out, void *hip_stream);
int syldet_sinc_resampler_flush_device(syldet_sinc_resampler_t *r, float *d_out, int64_t out_stride, int64_t *n_out, void *hip_stream);
int syldet_sinc_resample(syldet_sinc_resampler_t *r, const float *in, int64_t n_in, int64_t in_stride, float *out,
                         int64_t out_stride, int64_t *n_out);
int syldet_sinc_resampler_flush(syldet_sinc_resampler_t *r, float *out, int64_t out_stride, int64_t *n_out);

/* ---- packed recordings: many recordings of different lengths through one bank ----
 * The reference's tool opens one file after another and runs each file's tracks alone (SyllableDetectorCLI/main.swift:63-130).
 * A run's results do not depend on where it starts as long as the start is a multiple of hop (evaluation e reads samples
 * [e hop, (e + T - 1) hop + gap + W) of its row), so recordings laid end to end in a bank's rows, each from a multiple of hop, go
 * through syldet_run_device* unchanged: recording k at row offset o_k has its evaluation e at row evaluation o_k / hop + e, with
 * the values it would have had alone -- bit for bit on the fold kernel, the generic engine and the 1024-point kernel; the
 * pass-scaled fused kernels and the wide engine keep their 1e-5 (1e-2) contract, not bit identity (their scale is per pass).
 * Row evaluations outside every [first_eval, first_eval + n_evals) straddle two recordings or a pad and mean nothing.
 * THE COLUMNS follow the same rule (frame j reads samples [j hop, j hop + gap + W) of its row): syldet_spectrogram_device on the
 * packed rows gives recording k's columns at row frames [first_eval, first_eval + syldet_count_frames(h, n_k)), with the values
 * syldet_spectrogram_device gives on that recording alone -- bit for bit on the fold kernel and the generic engine; row frames
 * outside those ranges straddle two recordings or a pad.
 * THE PLAN (host only, no device is touched), for K recordings of n_samples[k] samples on the C channels of h:
 *   P_k       = ceil(n_k / hop) hop                        the padded length
 *   n_evals_k = max(0, syldet_count_evals(h, n_k))
 *   recordings are placed in order of P_k descending, ties by index ascending; each goes to the ELIGIBLE row with the least
 *   samples placed so far (its fill), ties to the lowest row; slots[k].offset = that fill (a multiple of hop), and the row's fill
 *   grows by P_k;  slots[k].first_eval = offset / hop;  slots[k].n_samples = n_k
 *   *row_samples = the greatest fill, rounded up to a multiple of 8 (rows stay whole 4-byte words as int16 and 16-byte quads as fp32)
 *   *row_evals   = max(0, syldet_count_evals(h, *row_samples)); first_eval + n_evals <= *row_evals for every recording that has an
 *                  evaluation (one without may lie behind the row's last evaluation: nothing of it is ever read)
 *   *fill        = sum n_k / (C *row_samples)   (0 where *row_samples is 0)
 * Guarantee (greedy placement): *row_samples <= ceil(sum P_k / C) + max P_k + 7 where every row is eligible for every recording
 * (with several networks: for each network's own rows and recordings).
 * Eligibility: on a plain bank every row (network must be NULL or all zeros); on a syldet_create_multi / syldet_create_mixed bank
 * recording k may only go to rows whose channel_net equals network[k] (network == NULL: SYLDET_ERR_INVALID_ARGUMENT; a network no
 * row runs: SYLDET_ERR_UNSUPPORTED, syldet_last_error names it).  Zero-length recordings are legal (a slot without samples or
 * evaluations).  SYLDET_ERR_INVALID_ARGUMENT: a NULL handle, n_recordings < 0, a NULL array with n_recordings > 0, a negative length
 * or network.  slots, row_samples, row_evals and fill may each be NULL.  A sharded bank (syldet_sharded_t) has no packed form: no
 * entry point takes one, and the language bindings answer SYLDET_ERR_UNSUPPORTED.
 * THE HANDLE keeps the plan and its tables on the device of h (h must outlive it), so that the device calls are launches only:
 * they do not allocate, synchronise or copy -- with one exception, stated here: the sources (src_offset, src_step: host arrays of
 * K entries) are kept by the handle, and a load whose sources differ from the kept ones (the first load always) waits for the
 * stream of the handle's last load and uploads them with one blocking copy first.  Loading again from the same layout -- the
 * next batch of a tool that reuses its upload buffer, a measurement loop -- is one launch.
 *   syldet_recordings_load_device*   sample i of recording k is d_src[src_offset[k] + i src_step[k]] (step 1: a planar recording;
 *       step n: one track of an n-track file uploaded as its WAV stores it -- the call is also the de-interleave; src_step NULL:
 *       all 1; steps >= 1, offsets >= 0).  Writes every element [0, row_samples) of every row of d_rows [C][channel_stride]: a
 *       recording's sample, or +0 in the pads behind each recording and in the tail of shorter rows (junk evaluations read the
 *       pads: anything non-finite there would send them through the exact recomputation); [row_samples, channel_stride) is left
 *       untouched.  Any hop, any source offset, any step; 16-byte accesses where the rows are 16-byte aligned (base and stride)
 *       and, for the reads, 16, 8 or 4 bytes an access where a recording is contiguous, as its source address allows -- one
 *       element at a time elsewhere.  ("recordings_load_kernel")
 *   syldet_recordings_events_device  d_outputs [C][row_evals][n_out] and d_flags [C][row_evals] as syldet_run_device* wrote them
 *       for the packed rows -> for recording k exactly what syldet_detections_device gives on that recording's flags alone
 *       (idx = first_index + e hop with e counted from the recording's first evaluation, debounce_until = -1 at its start):
 *       d_indices [K][capacity], d_counts [K] (may exceed capacity), and d_values [K][capacity][n_out], the outputs of each
 *       detection's evaluation.  d_outputs and d_values may be NULL together (indices only).  One wave a recording, the scan of
 *       syldet_detections_device; row evaluations outside the recordings are never read.  ("recordings_events_kernel")
 * Statuses of the device calls, before any device is touched: SYLDET_ERR_INVALID_ARGUMENT for a NULL handle or pointer (but
 * the optional ones), channel_stride < row_samples, a negative offset, a step < 1, capacity < 0, d_outputs without d_values or
 * the reverse.  The handle follows the bank's rule of one stream at a time.                                                   */
typedef struct {
    int32_t row;             /* the bank row the recording lies in */
    int64_t offset;          /* its first sample in that row, a multiple of hop */
    int64_t first_eval;      /* offset / hop: the row evaluation that is its evaluation 0 */
    int64_t n_evals;
    int64_t n_samples;
} syldet_slot_t;
typedef struct syldet_recordings syldet_recordings_t;
int syldet_recordings_plan(const syldet_t *h, const int64_t *n_samples, const int32_t *network, int32_t n_recordings,
                           syldet_slot_t *slots, int64_t *row_samples, int64_t *row_evals, double *fill);
/* the same plan from the host alone, for a machine without a device: a bank of n_channels channels on cfg's evaluation clock (any
 * of the bank's networks: they share it); channel_net as syldet_create_multi / syldet_create_mixed take it, NULL for a plain bank */
int syldet_recordings_plan_of_config(const syldet_config_t *cfg, int32_t n_channels, const int32_t *channel_net, const int64_t *n_samples,
                                     const int32_t *network, int32_t n_recordings, syldet_slot_t *slots, int64_t *row_samples,
                                     int64_t *row_evals, double *fill);
int syldet_recordings_create(const syldet_t *h, const int64_t *n_samples, const int32_t *network, int32_t n_recordings,
                             syldet_recordings_t **out);
int syldet_recordings_destroy(syldet_recordings_t *r);
/* slots: n_recordings entries, in the caller's order */
int syldet_recordings_slots(const syldet_recordings_t *r, syldet_slot_t *slots);
int syldet_recordings_shape(const syldet_recordings_t *r, int32_t *n_recordings, int64_t *row_samples, int64_t *row_evals, double *fill);
int syldet_recordings_load_device(syldet_recordings_t *r, const float *d_src, const int64_t *src_offset, const int32_t *src_step,
                                  float *d_rows, int64_t channel_stride, void *hip_stream);
int syldet_recordings_load_device_s16(syldet_recordings_t *r, const int16_t *d_src, const int64_t *src_offset, const int32_t *src_step,
                                      int16_t *d_rows, int64_t channel_stride, void *hip_stream);
int syldet_recordings_events_device(syldet_recordings_t *r, const float *d_outputs, const uint8_t *d_flags, double debounce_seconds,
                                    int64_t *d_indices, float *d_values, int64_t capacity, int64_t *d_counts, void *hip_stream);

/* ---- packed recordings at other rates: convert as the rows load ----
 * An archive is rarely at one rate.  These calls are syldet_recordings_load_device for recordings that are each at a rate of their
 * own: every recording of the plan is brought to the network's rate by the band-limited converter (the sinc convention above)
 * straight into its place in the rows, in ONE launch ("recordings_load_sinc_kernel"), instead of one
 * syldet_convert_rate_sinc_device call a recording into scratch rows and a load that copies them again.
 *   src_samples[k]   the length of recording k at its own rate src_rate[k]; sample j of it is d_src[src_offset[k] + j src_step[k]],
 *                    exactly as in syldet_recordings_load_device (the call is still the de-interleave)
 *   THE PLAN is made as before, from lengths at the network's rate `rate` (the bank's sampling rate): the caller passes
 *                    n_k = syldet_convert_rate_count(src_samples[k], src_rate[k], rate) to syldet_recordings_create, and the call
 *                    refuses (SYLDET_ERR_INVALID_ARGUMENT, syldet_last_error names the recording) any k whose slots[k].n_samples
 *                    differs from that count
 *   d_rows           always fp32 [C][channel_stride]; an int16 source means x * 2^-15, as everywhere else in the library
 * THE CONTRACT:
 *   a recording at another rate   for every k with src_rate[k] != rate and every i < n_k, d_rows[row_k][offset_k + i] holds the bits
 *       syldet_convert_rate_sinc_device (_s16) writes at output i when it is given that recording alone as one contiguous row
 *       with the same (zero_crossings, beta, rolloff): the same table, the same fp64 position p_i = (double)i * src_rate[k] / rate
 *       with i counted from the recording's start, the same taps in the same order
 *   a recording at the network's rate   where src_rate[k] == rate the samples are copied (widened for int16), not low-passed
 *   everywhere else   every other element of [0, row_samples) of every row is +0; [row_samples, channel_stride) is left untouched
 *   downstream   by the packed-rows property above, on the fold kernel, the generic engine and the 1024-point kernel each
 *       recording's outputs and flags are then bit for bit those of converting it alone and running it alone
 * Statuses, decided before any device is touched, in this order: the argument checks of syldet_recordings_load_device (src_samples
 * and src_rate may be NULL only without recordings); SYLDET_ERR_INVALID_ARGUMENT for src_samples[k] < 0 or a rate that is not
 * positive and finite; the statuses of syldet_convert_rate_sinc_device for zero_crossings, beta or rolloff out of range; then, for
 * each recording in turn, SYLDET_ERR_UNSUPPORTED for src_rate[k] / rate outside [1/16, 16] or H > 65536 (only where src_rate[k] !=
 * rate) and SYLDET_ERR_INVALID_ARGUMENT for a length that differs from the plan's -- syldet_last_error names the recording.
 * The launch rule is the plain load's: the handle keeps the sources, which here include src_samples, src_rate and the quality (kept
 * apart from the plain load's, so the two may take turns); a load whose sources differ from the kept ones waits for the stream of
 * the handle's last converting load and uploads its tables -- K + C words, never a list of workgroups -- with one blocking copy;
 * the same layout again is one launch without allocation, synchronisation or copy.  The filter's table comes from the (Z, beta)
 * cache of syldet_convert_rate_sinc_device, with its blocking copy on first use.                                               */
int syldet_recordings_load_sinc_device(syldet_recordings_t *r, const float *d_src, const int64_t *src_offset, const int32_t *src_step,
                                       const int64_t *src_samples, const double *src_rate, int32_t zero_crossings, double beta,
                                       double rolloff, float *d_rows, int64_t channel_stride, void *hip_stream);
int syldet_recordings_load_sinc_device_s16(syldet_recordings_t *r, const int16_t *d_src, const int64_t *src_offset, const int32_t *src_step,
                                           const int64_t *src_samples, const double *src_rate, int32_t zero_crossings, double beta,
                                           double rolloff, float *d_rows, int64_t channel_stride, void *hip_stream);

/* ---- packed recordings: the files' own sample formats ----
 * The reference asks AVFoundation for 32-bit float linear PCM whatever a file holds (audioSettings, Common/SyllableDetector.swift:19-23);
 * the calls below stand in for that delivery: the source of a load is the files' own bytes, and every recording of a plan is
 * decoded from its own little-endian format, de-interleaved and placed in the fp32 rows in ONE launch -- a batch of 16- and 24-bit
 * files is uploaded as it is stored, not widened on the host and uploaded as fp32.
 * THE CONVENTION (csrc/pcm_values.hpp: one text for the host, the kernels and a stand-alone test):
 *   SYLDET_PCM_U8   1 byte   (float)(b - 128) * 2^-7
 *   SYLDET_PCM_S16  2 bytes  (float)v * 2^-15
 *   SYLDET_PCM_S24  3 bytes  (float)v * 2^-23      (v sign-extended from bit 23; exact in fp32)
 *   SYLDET_PCM_S32  4 bytes  (float)v * 2^-31      (= (float)((double)v / 2^31): a power-of-two scale commutes with the rounding)
 *   SYLDET_PCM_F32  4 bytes  the bits, copied (NaN payloads included)
 *   SYLDET_PCM_F64  8 bytes  (float)d, round to nearest even, fp32 subnormal results kept
 * -- the values the tool's WAV reader gives for the same bytes.  Little endian only.
 *   syldet_pcm_sample_bytes   the bytes of one sample; 0 for an unknown format
 *   syldet_pcm_decode         out[i] = the `format` value at bytes + i byte_step for i < n (byte_step >= the sample's bytes; any
 *       address: the host reads byte-wise).  SYLDET_ERR_INVALID_ARGUMENT for an unknown format, n < 0, a NULL array with n > 0, a
 *       step below the sample's bytes.  Host only.
 * THE DEVICE CALLS.  Sample i of recording k is the src_format[k] value at byte d_src + src_byte_offset[k] + i src_byte_step[k]; a
 * step of tracks * sample_bytes takes one track of an interleaved file as its `data` chunk stores it (src_byte_step NULL: every
 * recording contiguous).  d_src holds src_bytes bytes.
 *   syldet_recordings_load_pcm_device        every element [0, row_samples) of every row holds, bit for bit, what
 *       syldet_recordings_load_device writes from the fp32 array syldet_pcm_decode makes of the same bytes -- +0 in the pads and in
 *       empty rows included; [row_samples, channel_stride) is left untouched.  ("recordings_load_pcm_kernel": the grid and tile
 *       walk of recordings_load_kernel; a contiguous recording is read 8 (S16), 12 (S24), 16 (S32, F32), 32 (F64) or 4 (U8) bytes
 *       for four samples as its address allows, everything else sample by sample)
 *   syldet_recordings_load_sinc_pcm_device   the bits of syldet_recordings_load_sinc_device on those decoded fp32 arrays: the same
 *       table, the same fp64 positions, the same taps; a recording at the network's rate is decoded and copied
 * Reads: no byte outside the bytes of the recordings' own samples is read, and no access of several bytes is off a multiple of
 * its size (a group of four contiguous S24 samples: exactly its 12 bytes, from a multiple of 4).
 * Statuses, decided before any device is touched, in this order: the argument checks of syldet_recordings_load_device (offsets >= 0,
 * steps >= 1, ...); then SYLDET_ERR_INVALID_ARGUMENT, syldet_last_error naming the recording, for an unknown format, a
 * src_byte_step[k] below the sample's bytes, an address d_src + src_byte_offset[k] or a step that is no multiple of the sample's
 * size for S16, S32, F32 or F64 (U8 and S24 take any), a recording whose last sample byte lies at or beyond src_bytes (the plan's
 * n_samples of them; for the converting form src_samples[k]); then, for the converting form, the statuses of
 * syldet_recordings_load_sinc_device in its order.  syldet_pcm_check_sources makes the checks of this paragraph from the host alone
 * (n_samples: the samples read of each recording; src: the address d_src will have, never read).
 * The launch rule is the existing one: the handle keeps the sources, with the formats and the unit (bytes or elements) part of the
 * comparison, in the tables of the plain and of the converting load; the same layout again is one launch without allocation,
 * synchronisation or copy, and these calls and the four above may take turns on one handle, each writing its own bits.          */
#define SYLDET_PCM_U8  1
#define SYLDET_PCM_S16 2
#define SYLDET_PCM_S24 3
#define SYLDET_PCM_S32 4
#define SYLDET_PCM_F32 5
#define SYLDET_PCM_F64 6
int32_t syldet_pcm_sample_bytes(int32_t format);
int syldet_pcm_decode(int32_t format, const void *bytes, int64_t n, int64_t byte_step, float *out);
int syldet_pcm_check_sources(const void *src, int64_t src_bytes, const int64_t *src_byte_offset, const int32_t *src_byte_step,
                             const int32_t *src_format, const int64_t *n_samples, int32_t n_recordings);
int syldet_recordings_load_pcm_device(syldet_recordings_t *r, const void *d_src, int64_t src_bytes, const int64_t *src_byte_offset,
                                      const int32_t *src_byte_step, const int32_t *src_format, float *d_rows, int64_t channel_stride,
                                      void *hip_stream);
int syldet_recordings_load_sinc_pcm_device(syldet_recordings_t *r, const void *d_src, int64_t src_bytes, const int64_t *src_byte_offset,
                                           const int32_t *src_byte_step, const int32_t *src_format, const int64_t *src_samples,
                                           const double *src_rate, int32_t zero_crossings, double beta, double rolloff, float *d_rows,
                                           int64_t channel_stride, void *hip_stream);

/* ---- packed recordings: every recording's output track and trigger track ----
 * The two per-sample products of a run -- the Simulator's output track (syldet_trace*) and the TTL trigger track
 * (syldet_trigger*) -- for every recording of a packed bank, written straight to a destination of the recording's own, in a
 * fixed number of launches whatever K is.  d_outputs is [C][row_evals][n_out] and d_flags [C][row_evals], as syldet_run_device*
 * wrote them for the packed rows.
 * DESTINATIONS mirror the loads' sources: element i of recording k, 0 <= i < n_k = slots[k].n_samples, goes to
 * d_dst[dst_offset[k] + i dst_step[k]] (host arrays of K entries; dst_step NULL: all 1).  Step 1 is a planar track; step n with
 * offsets base + t writes track t of an n-track file's frames, so the call is also the interleave.  No other element of d_dst is
 * written; dst_elements is the size of d_dst in elements.  Destinations of different recordings that share an element are the
 * caller's error: which value lands there is unspecified, and nothing outside d_dst is touched.
 * THE CONTRACT is identity with the calls for one recording:
 *   trace     recording k's elements are, bit for bit, what syldet_trace_device (_s16) writes for n_samples = n_k when it is given
 *             that recording's n_evals_k outputs alone, on a one-channel handle of the recording's network: the hold starts at
 *             first_index counted from the recording's own sample 0, samples behind first_index + n_evals_k hop are 0, and the
 *             division is by Float(thresholds[output]) of the network of the recording's row (plain, multi-network and mixed banks)
 *   trigger   recording k's elements are those of syldet_trigger_device (_s16) on that recording's flags alone with n_samples =
 *             n_k: the buffers b(e) = (D + e hop - 1) / L are counted with e and the samples from the recording's own start, a
 *             pulse armed near a recording's end is cut at n_k and never reaches the next recording of the row, and a row
 *             evaluation outside every recording is never read
 *   onsets    d_indices [K][capacity] and d_counts [K] are those of syldet_trigger_onsets_device on the recording alone; the
 *             counts may exceed the capacity, only the first min(count, capacity) indices are written
 *   a recording without samples writes nothing; one without evaluations writes zeros.
 * Statuses, decided before any device is touched: SYLDET_ERR_INVALID_ARGUMENT for a NULL handle or required pointer, `output`
 * outside [0, outputs), the limits of buffer_length, width_samples and latency_samples stated for syldet_trigger*, a negative
 * offset, a step < 1, capacity < 0, dst_elements < 0, and any k with n_k > 0 and dst_offset[k] + (n_k - 1) dst_step[k] >=
 * dst_elements (syldet_last_error names the recording).
 * THE LAUNCH RULE is the loads': the handle keeps the destination layout (dst_offset, dst_step), apart from the loads' sources,
 * so loads and track calls may take turns.  A call whose layout differs from the kept one (the first always) waits for the
 * stream of the handle's last track call and uploads the layout once, with a blocking copy; the same layout again is launches
 * only, without allocation, synchronisation or copy.  One layout is kept for the trace and the trigger calls together (a tool
 * writes both products to buffers of one shape); calls with layouts of their own may alternate, each then uploads.  The trigger
 * calls need a table last_seen per recording, B'_k = ceil((n_k + L - 1) / L) entries, the recordings' tables end to end: a
 * prefix of K + 1 entries is uploaded when buffer_length changes, and the tables are scratch the handle keeps and grows -- the
 * exception already stated for syldet_trigger*.  The first trace of an output uploads the bank's threshold table of that
 * output, as syldet_trace* does.  Launches, by the names syldet_timings lists:
 *   trace           "recordings_trace_kernel"
 *   trigger track   "recordings_trigger_scan_kernel", "recordings_trigger_kernel"
 *   onsets          "recordings_trigger_scan_kernel", "recordings_trigger_onsets_kernel"
 * The expansion kernels are balanced by rows, not by recordings; where dst_step is 1 they store 16 bytes at a time in groups
 * aligned to the destination (a recording's head and tail element by element), for any other step element by element.  The
 * scan is one workgroup a recording: no workgroup waits for another.  A sharded bank has no packed form, as before.
 * STREAMS AND THREADS.  The handle waits only for the stream of its LAST track call before it rewrites a table (the loads have
 * the same rule), so track calls of one handle on different streams must be ordered by the caller: with a kernel of an earlier
 * call still running on another stream, a call with a changed layout or buffer_length may overwrite what that kernel reads.
 * The track calls also WRITE to the bank h the handle was created from, although syldet_recordings_create takes it const: the
 * first trace of an output makes the bank's threshold table of that output, and every call records into the bank's profile
 * (syldet_profile).  So the bank's rule of one caller at a time covers them too: two syldet_recordings_t of one bank, or one of
 * them and the bank itself, must not be used from two threads at once.                                                        */
int syldet_recordings_trace_device(syldet_recordings_t *r, const float *d_outputs, int32_t output, float *d_dst, int64_t dst_elements,
                                   const int64_t *dst_offset, const int32_t *dst_step, void *hip_stream);
int syldet_recordings_trace_device_s16(syldet_recordings_t *r, const float *d_outputs, int32_t output, int16_t *d_dst, int64_t dst_elements,
                                       const int64_t *dst_offset, const int32_t *dst_step, void *hip_stream);
int syldet_recordings_trigger_device(syldet_recordings_t *r, const uint8_t *d_flags, int32_t buffer_length, int64_t width_samples,
                                     int64_t latency_samples, float *d_dst, int64_t dst_elements, const int64_t *dst_offset,
                                     const int32_t *dst_step, void *hip_stream);
int syldet_recordings_trigger_device_s16(syldet_recordings_t *r, const uint8_t *d_flags, int32_t buffer_length, int64_t width_samples,
                                         int64_t latency_samples, int16_t *d_dst, int64_t dst_elements, const int64_t *dst_offset,
                                         const int32_t *dst_step, void *hip_stream);
int syldet_recordings_trigger_onsets_device(syldet_recordings_t *r, const uint8_t *d_flags, int32_t buffer_length, int64_t width_samples,
                                            int64_t latency_samples, int64_t *d_indices, int64_t capacity, int64_t *d_counts,
                                            void *hip_stream);

/* ---- packed recordings: every recording's level meters ----
 * The third batch product of a run -- the level meters of a row (syldet_levels*, syldet_output_levels*) -- for every recording
 * of a packed bank, in a fixed number of launches whatever K is.  L = buffer_length, P = buffers_per_reading, with the limits
 * stated for syldet_levels*.
 * THE LAYOUT (syldet_recordings_levels_layout: host only, no device is touched): recording k of n_k = slots[k].n_samples samples
 * has M_k = syldet_levels_count(n_k, L, P) readings (0 for a recording without samples); they are elements
 * [reading_first[k], reading_first[k + 1]) of the result arrays, in the caller's order of recordings, and *n_readings =
 * reading_first[K].  reading_first (K + 1 entries) may be NULL.
 *   syldet_recordings_levels_device*         d_rows [C][channel_stride] fp32 or (_s16) int16: the rows syldet_recordings_load_device*
 *       or syldet_recordings_load_sinc_device* wrote -> d_mean_square [n_readings] fp64
 *   syldet_recordings_output_levels_device   d_outputs [C][row_evals][n_out] as syldet_run_device* wrote it for the packed rows
 *       -> d_levels [n_readings] fp32
 * `capacity` is the size of the result array in elements; no element past n_readings is written.
 * THE CONTRACT is identity with the calls for one recording:
 *   input meter    recording k's M_k mean squares are, bit for bit, what syldet_levels_device (_s16) writes for that recording
 *       alone (a one-channel handle, n_samples = n_k, the same L and P): buffers are counted from the recording's own sample 0,
 *       buffer b is its samples [b L, min((b + 1) L, n_k)), the last one divides by its own length, sum_squares_tree runs in
 *       index order from the recording's start (not the row's), and P is clamped to the recording's own buffer count as the
 *       one-recording call clamps it.  A reading is NaN exactly where the one-recording call's is (the payload bits of a NaN are
 *       not part of the contract).  Nothing outside a recording is ever read as part of it -- not a pad, not the next recording
 *       of the row, not the tail of a short row: a short last buffer is masked at n_k, not trusted to find zeros.
 *   output meter   recording k's M_k values are those of syldet_output_levels_device on the recording's n_evals_k outputs alone
 *       with n_samples = n_k: the evaluation range of reading m is syldet_levels_eval_range's for (n_k, n_evals_k), read at row
 *       evaluations first_eval_k + e; 0 for a reading without an evaluation.  Row evaluations outside every recording are never
 *       read.  Plain, multi-network and mixed banks alike: `output` is checked against, and n_out taken from, the bank's outputs,
 *       as syldet_output_levels_device does.
 * Statuses, decided before any device is touched: SYLDET_ERR_INVALID_ARGUMENT for a NULL handle or pointer (d_outputs may be NULL
 * where row_evals is 0), channel_stride < row_samples, an L that is not a power of two in [8, 4096], P < 1, `output` outside
 * [0, outputs), and capacity < n_readings (syldet_last_error says how many are needed).  A refused call writes nothing.
 * THE LAUNCH RULE is the tracks': the handle keeps (L, P) and, on the device, the reading prefix of that pair (K + 1 words, and
 * the same K starts once more in the order of the plan's table), apart from the tracks' and the loads' tables.  A call whose
 * (L, P) differs from the kept pair (the first always) waits for the stream of the handle's last levels call and uploads once,
 * with a blocking copy; the same pair again is launches only, without allocation, synchronisation or copy.  One pair is kept for
 * the two meters together.  No scratch: a reading that crosses workgroups is made with one vector atomic maximum a workgroup on
 * the bits of its mean squares (non-negative doubles order as unsigned integers; a NaN first value goes in as the canonical quiet
 * NaN, above +inf), over a table set to +0 first -- exact, the same bits whatever the order, and no workgroup waits for another.
 * Launches, by the names syldet_timings lists:
 *   input meter    "recordings_levels_zero_kernel" (only where rows are longer than one tile of 8192 samples: the +0 the atomics
 *                  need), "recordings_levels_in_kernel"
 *   output meter   "recordings_levels_out_kernel"
 * The input meter is balanced by rows, not by recordings; it loads 16 bytes a lane where a recording's first sample is 16-byte
 * aligned in device memory, 8 or 4 bytes an access where it is aligned to that, one element at a time elsewhere (and for a
 * recording's last partial group).  A sharded bank has no packed form, as before.
 * STREAMS AND THREADS: as stated for the tracks.  Levels calls of one handle on different streams must be ordered by the caller,
 * and every call records into the profile of the bank h the handle was created from, so the bank's rule of one caller at a time
 * covers them too.                                                                                                          */
int syldet_recordings_levels_layout(const syldet_recordings_t *r, int32_t buffer_length, int64_t buffers_per_reading,
                                    int64_t *reading_first, int64_t *n_readings);
int syldet_recordings_levels_device(syldet_recordings_t *r, const float *d_rows, int64_t channel_stride, int32_t buffer_length,
                                    int64_t buffers_per_reading, double *d_mean_square, int64_t capacity, void *hip_stream);
int syldet_recordings_levels_device_s16(syldet_recordings_t *r, const int16_t *d_rows, int64_t channel_stride, int32_t buffer_length,
                                        int64_t buffers_per_reading, double *d_mean_square, int64_t capacity, void *hip_stream);
int syldet_recordings_output_levels_device(syldet_recordings_t *r, const float *d_outputs, int32_t output, int32_t buffer_length,
                                           int64_t buffers_per_reading, float *d_levels, int64_t capacity, void *hip_stream);

/* ---- threshold calibration: score a run against labelled times ----
 * Which threshold to ship, and how late and how jittery the trigger is at it: the reference leaves the question to MATLAB
 * (convert_to_text.m:70-72 only copies trigger_thresholds in).  Here the outputs of a run, which are on the device already, are
 * scored for K candidate thresholds in one launch.  Under debounce hits and false positives do not move monotonically with the
 * threshold (a low one fires early on noise and the debounce swallows the real crossing), so every threshold runs the debounce
 * scan of TrackDetector.swift:65-100 for itself.  THE CONVENTION is the library's own (as the sinc converter's and the meters'):
 * A DETECTOR is one channel of a bank, or one recording of a syldet_recordings_t.  Its evaluations e = 0 .. E-1 have the sample
 * numbers idx_e = first_index + e hop; for a recording e and the samples count from its own start (the numbering of
 * syldet_detections_device and syldet_recordings_events_device).  For one detector, one output o and one threshold theta (a double):
 *   flag      flag_e = Double(out[e][o]) >= theta.  NaN never fires.  Only output o counts, whatever the handle's rule.
 *   debounce  until = -1 at the detector's start; a detection is emitted iff flag_e && until < idx_e, and then
 *             until = idx_e + Int(debounce_seconds * samplingRate).
 *   labels    detector d has sorted sample numbers t_0 < .. < t_{n-1} and every detector the tolerance of m >= 0 samples.  The
 *             windows [t_j - m, t_j + m] must be disjoint: t_{j+1} - t_j > 2 m (else SYLDET_ERR_INVALID_ARGUMENT, and
 *             syldet_last_error names the detector and the label).  A label may lie before sample 0 or behind the detector's end.
 *   class     each emitted detection falls in exactly one: in window j and j not yet hit at this theta -- a HIT, which adds
 *             idx - t_j to the offset sum and its square to the squared-offset sum; in window j and j already hit -- a REPEAT;
 *             in no window -- a FALSE POSITIVE.
 *   result    table [D][K][6], int64, the columns SYLDET_SCORE_* below.  Always detections = hits + false_positives + repeats;
 *             the misses are n_d - hits.  Integer arithmetic throughout: device, host and any model of the above agree exactly.
 * Limits: 1 <= K <= SYLDET_SCORE_MAX_THRESHOLDS; thresholds may be +-inf or beyond FLT_MAX, NaN is refused; 0 <= m <= 2^20;
 * debounce_seconds * samplingRate must be a number of magnitude below 2^62.
 * (The device compares in fp32 against the smallest float >= theta, +inf beyond FLT_MAX, computed at creation: exact, because
 * float -> double is exact.)
 *   syldet_scorer_create   h: the bank; r: NULL (one detector a channel, D = its channels) or a packed-recordings handle of h
 *       (D = its recordings); thresholds [K]; labels: all detectors' labels end to end, detector d's at [label_begin[d],
 *       label_begin[d + 1]) (label_begin [D + 1], starting at 0 and not decreasing; labels may be NULL where there are none).
 *       Everything is validated before any device is touched; then thresholds, labels and, for recordings, the slots' (row,
 *       first_eval, n_evals) are uploaded once.  h, and r if given, must outlive the scorer.
 *   syldet_score_device    d_outputs as syldet_run_device* wrote them: [C][n_evals][n_out] without r; with r n_evals must equal
 *       row_evals, and recording k reads only its own [first_eval, first_eval + n_evals_k) of its row.  d_table [D][K][6].  One
 *       launch ("score_kernel": one wave a detector and group of 64 thresholds, a lane a threshold); it never allocates,
 *       synchronises or copies, and follows the bank's rule of one stream at a time.  SYLDET_ERR_INVALID_ARGUMENT: NULL pointers,
 *       output outside [0, n_out), n_evals < 0, a wrong n_evals with r.  Plain, multi-network and mixed banks; a sharded bank
 *       has none.  One detector is one sequential chain: it is not split along time, the parallelism is detectors x groups.
 *   syldet_score_host      host only: one detector in plain C++ (the text the kernel's lanes run, one threshold after another):
 *       evaluation e's value is values[e value_stride]; table [K][6].
 *   syldet_score_choose    host only: sums table [D][K][6] over the detectors (n_labels [D]: each detector's label count) into
 *       totals [K][6] (may be NULL); cost_k = misses_k + false_positive_cost (false_positives_k + repeats_k) in double (costs
 *       [K], may be NULL; false_positive_cost is not NaN); *best = the lowest k of the smallest cost.                            */
#define SYLDET_SCORE_DETECTIONS         0
#define SYLDET_SCORE_HITS               1
#define SYLDET_SCORE_FALSE_POSITIVES    2
#define SYLDET_SCORE_REPEATS            3
#define SYLDET_SCORE_SUM_OFFSET         4
#define SYLDET_SCORE_SUM_OFFSET_SQUARED 5
#define SYLDET_SCORE_COLUMNS            6
#define SYLDET_SCORE_MAX_THRESHOLDS     4096
#define SYLDET_SCORE_MAX_TOLERANCE      1048576
typedef struct syldet_scorer syldet_scorer_t;
int syldet_scorer_create(const syldet_t *h, const syldet_recordings_t *r, const double *thresholds, int32_t n_thresholds,
                         const int64_t *labels, const int64_t *label_begin, int64_t tolerance_samples, double debounce_seconds,
                         syldet_scorer_t **out);
int syldet_scorer_destroy(syldet_scorer_t *s);
int syldet_scorer_shape(const syldet_scorer_t *s, int32_t *n_detectors, int32_t *n_thresholds, int64_t *n_labels);
int syldet_score_device(syldet_scorer_t *s, const float *d_outputs, int64_t n_evals, int32_t output, int64_t *d_table,
                        void *hip_stream);
int syldet_score_host(const float *values, int64_t n_evals, int64_t value_stride, const double *thresholds, int32_t n_thresholds,
                      const int64_t *labels, int64_t n_labels, int64_t tolerance_samples, int64_t first_index, int64_t hop,
                      int64_t debounce_frames, int64_t *table);
int syldet_score_choose(const int64_t *table, int32_t n_detectors, int32_t n_thresholds, const int64_t *n_labels,
                        double false_positive_cost, int32_t *best, int64_t *totals, double *costs);

/* ---- event-aligned windows: spectrogram, output and audio at each event ----
 * The figure a lab draws to judge a detector is the aligned stack: the spectrogram around every detection (or every label), one
 * window an event, their mean (a sharp mean is low jitter), and the same stack of the network's output.  The reference has no
 * counterpart; the arrays it would be cut from -- columns, outputs, samples -- are on the device already, and these calls cut
 * every event's window out of them in one launch, for a bank's channels or for all recordings of a packed plan.  THE CONVENTION
 * is the library's own (as the meters' and the scorer's):
 * A DETECTOR is a channel of a bank, or a recording of a packed-recordings handle (the scorer's definition).
 * An EVENT is any int64 sample number s counted from the detector's own start, |s| < 2^62: a detection index of
 *   syldet_detections_device or syldet_recordings_events_device, a label, anything else -- in any order, repeated, before 0 or
 *   behind the detector's end.
 * A SOURCE is one of three arrays that lie on the device, each of `width` floats a UNIT, with the anchor rule
 *   u0 = floor((s - origin) / step)   (a floor also for a negative numerator):
 *     source                array                                                      unit        width  origin      step  a detector's units U_d
 *     SYLDET_ALIGN_COLUMNS  [C][n_frames][bins] as syldet_spectrogram_device wrote it  frame       bins   gap + W     hop   syldet_count_frames of its samples
 *     SYLDET_ALIGN_OUTPUTS  [C][n_evals][n_out] as syldet_run_device* wrote it         evaluation  n_out  first_index hop   its n_evals
 *     SYLDET_ALIGN_SAMPLES  fp32 rows [C][channel_stride]                              sample      1      0           1     its n_samples
 *   For a detection s = first_index + e hop the anchor evaluation is e and the anchor frame is e + T - 1, the newest column the
 *   network saw: with before = T - 1, after = 0 a COLUMNS window is exactly the network's input in spectrogram values.
 *   (A channel of a bank has the n_units of the call; a recording its own part of its row.)
 * THE WINDOW of an event is the units u0 - before .. u0 + after, n = before + after + 1 of them; 0 <= before, after and
 *   n width <= SYLDET_ALIGN_MAX_WINDOW.  An element whose unit lies in [0, U_d) of its own detector is PRESENT and is a bit copy
 *   of the source; every other element is the caller's `fill` float (NaN, 0, ...).  For a packed recording with slot sl, unit u is
 *   unit sl.first_eval + u of row sl.row for COLUMNS and OUTPUTS, and sample sl.offset + u of it for SAMPLES: frames and
 *   evaluations between two recordings, pads and the next recording of the row are never read.
 * THE RESULT is d_windows [N][n][width] fp32; detector d's j-th event is window event_begin[d] + j.  event_begin is a host array of
 *   D + 1 entries, from 0 and not decreasing (as the scorer's label_begin), N = event_begin[D].  The events are on the device, at
 *   d_events[d event_stride + j] -- the [D][capacity] tables of the detection calls as they are -- or, with event_stride == 0,
 *   flat at d_events[event_begin[d] + j].  Every element of d_windows is written exactly once, nothing behind N n width.
 * STACK STATISTICS.  group [D] (host, int32, 0 <= g < G) puts every detector on a stack.  A group's events are ordered by detector
 *   ascending, then event index ascending, and numbered i = 0, 1, ...  For every position p of the n width elements:
 *     count[g][p]   int64: the events of the group whose element p is present (by the window rule, whatever the value or the fill)
 *     sum[g][p], sumsq[g][p]   fp64, over those events IN BLOCKS OF SYLDET_ALIGN_BLOCK CONSECUTIVE i: inside a block the values
 *                   (their squares, taken in fp64: exact for an fp32 value, so a fused multiply-add changes nothing) are added one
 *                   after another in order, from +0.0; the blocks' results are added one after another in block order, from +0.0.
 *                   Absent elements add nothing; NaN propagates.
 *   A fixed tree: device, host and any model of the above agree to the bit.  Mean and variance are the caller's divisions.
 *   syldet_aligner_create    h: the bank; r: NULL (D = its channels) or a packed-recordings handle of h (D = its recordings).
 *       Everything is validated before any device is touched; for recordings the slots' (row, first unit, units) are uploaded
 *       once.  h, and r if given, must outlive the aligner.
 *   syldet_aligner_shape     D, n and width
 *   syldet_align_anchor      host only: origin, step and width of a source on h (each may be NULL)
 *   syldet_align_device      d_src: the source array, n_units units a row (with r: the rows' row_evals for OUTPUTS,
 *       syldet_count_frames(h, row_samples) for COLUMNS, row_samples for SAMPLES), rows row_stride ELEMENTS apart (0: n_units
 *       width; for SAMPLES the channel_stride).  One launch ("align_windows_kernel": a window is one contiguous span of the source
 *       copied to one contiguous span of d_windows with fill on either side -- csrc/align_span.hpp, one text for the kernel, the host
 *       and a stand-alone test; a wave takes a short window, a workgroup a long one; 16 bytes a lane where the destination's
 *       address allows, element by element at its ends and at the clipped ends of the span).
 *   syldet_align_stats_device   the statistics of the windows the aligner's LAST syldet_align_device call wrote (d_windows: that
 *       call's result, event_begin: that call's -- anything else is SYLDET_ERR_INVALID_ARGUMENT; the kernel left each window's
 *       present span with the aligner, which is what `count` goes by; only event_begin can be compared: a second windows call with
 *       the same event_begin but other events, another source or n_units replaces the spans, and statistics of the FIRST call's
 *       d_windows would then go by the wrong spans without a status -- take the statistics before the next windows call).  d_count, d_sum, d_sumsq [G][n][width].  Two launches
 *       ("align_stats_kernel": a thread owns a position of one block of a group and walks its windows in order;
 *       "align_combine_kernel": a group's blocks in order).
 *   syldet_align_host        host only, one detector in plain C++ (the text the kernel runs): src holds the detector's n_units
 *       units; windows [n_events][n][width]; present [n_events][2], may be NULL: each window's first present ELEMENT and the number
 *       of present elements.  origin in [0, 2^32), step in [1, 2^31).
 *   syldet_align_stats_host  host only, one group: the block tree over n_events windows of window_elements elements in the order
 *       given, present as syldet_align_host wrote it; count, sum, sumsq [window_elements].
 * Statuses, decided before any device is touched.  SYLDET_ERR_INVALID_ARGUMENT: a NULL handle or pointer (the device arrays may be
 * NULL where there is no event, d_src where n_units is 0), an unknown source, a negative before or after, a window above the limit, a wrong n_units with r,
 * a row_stride smaller than a row needs, an event_begin that does not start at 0 or that decreases, an event_stride that is not 0
 * and is smaller than a detector's event count, a group outside [0, G), G < 1.  SYLDET_ERR_UNSUPPORTED: COLUMNS on a mixed bank
 * of more than one class, as syldet_spectrogram* answers there (OUTPUTS and SAMPLES work on every kind of bank); more than
 * 2^31 - 1 windows or 2^40 window elements in one call.  A sharded bank
 * has none: no entry point takes one, and the language bindings answer SYLDET_ERR_UNSUPPORTED.
 * THE LAUNCH RULE is that of the recordings' load sources: the aligner keeps event_begin and, for the statistics, the group order
 * on the device.  A call whose host arrays differ from the kept ones (the first always) waits for the stream of the aligner's last
 * call, sizes what depends on them -- the spans [N], the order [N], the blocks' partials, scratch the aligner keeps and grows --
 * and uploads them with one blocking copy; the same arrays again are launches only: no allocation, no synchronisation, no copy.
 * One stream at a time, as the bank; every call records into the profile of h (syldet_profile), so the bank's rule of one caller
 * at a time covers the aligner too.                                                                                            */
#define SYLDET_ALIGN_COLUMNS    0
#define SYLDET_ALIGN_OUTPUTS    1
#define SYLDET_ALIGN_SAMPLES    2
#define SYLDET_ALIGN_MAX_WINDOW 1048576
#define SYLDET_ALIGN_BLOCK      256
typedef struct syldet_aligner syldet_aligner_t;
int syldet_aligner_create(const syldet_t *h, const syldet_recordings_t *r, int32_t source, int64_t before, int64_t after,
                          syldet_aligner_t **out);
int syldet_aligner_destroy(syldet_aligner_t *a);
int syldet_aligner_shape(const syldet_aligner_t *a, int32_t *n_detectors, int64_t *n_units_per_window, int32_t *width);
int syldet_align_anchor(const syldet_t *h, int32_t source, int64_t *origin, int64_t *step, int32_t *width);
int syldet_align_device(syldet_aligner_t *a, const float *d_src, int64_t n_units, int64_t row_stride, const int64_t *d_events,
                        int64_t event_stride, const int64_t *event_begin, float fill, float *d_windows, void *hip_stream);
int syldet_align_stats_device(syldet_aligner_t *a, const float *d_windows, const int64_t *event_begin, const int32_t *group,
                              int32_t n_groups, int64_t *d_count, double *d_sum, double *d_sumsq, void *hip_stream);
int syldet_align_host(const float *src, int64_t n_units, int32_t width, int64_t origin, int64_t step, int64_t before, int64_t after,
                      const int64_t *events, int64_t n_events, float fill, float *windows, int64_t *present);
int syldet_align_stats_host(const float *windows, const int64_t *present, int64_t n_events, int64_t window_elements, int64_t *count,
                            double *sum, double *sumsq);

/* ---- training: loss and gradient of a network over labelled recordings ----
 * The reference's detector is "a simple Matlab neural network trained using the training code"; its only bridge is
 * convert_to_text.m.  Everything training reads is on the device already -- the columns of syldet_spectrogram_device, labels as the
 * scorer takes them -- and the N x I input matrix is those columns repeated timeRange times.  These calls give loss and gradient
 * of the network's parameters over weighted, labelled evaluations straight from the columns; that matrix is never formed.  The
 * optimiser is the caller's, or the one of "training from the tool" below.  THE CONVENTION is the library's own (as the scorer's and the aligner's):
 * A DETECTOR, its evaluations e and their sample numbers idx_e = first_index + e hop are the scorer's; for a recording e and the
 *   samples count from its own start, and its evaluation e is evaluation slot.first_eval + e of row slot.row.  Evaluation e of a row
 *   reads the I = timeRange x bins contiguous floats from frame e of that row of the columns (the aligner's COLUMNS window with
 *   before = timeRange - 1, after = 0).
 * PARAMETERS: one flat fp32 vector theta of P = H I + H + O H + O elements: layer0.weights [H][I], layer0.biases [H],
 *   layer1.weights [O][H], layer1.biases [O], each weight block row-major as syldet_layer_t has it.  Everything else -- scaling,
 *   the input functions and their map parameters, the two transfer functions, the output maps -- is read from the bank's
 *   configuration at creation and is fixed.  theta comes with every call; the bank's own weights are never touched.
 * FORWARD: what the generic engine computes for an evaluation, from the linear columns: scaling (linear / log / dB), the input
 *   functions in file order (a normalize over range 0 fills -1, as the engines do), the two layers, the reverse output maps; all in
 *   fp32 (the first layer's products are summed frame by frame, then the frames), giving y_e[o].
 * TARGETS AND WEIGHTS: t [rows][n_evals][O] and w [rows][n_evals], fp32, on the device.  Evaluation e of a row is SELECTED iff
 *   w > 0; a NaN weight is not selected.  An unselected evaluation contributes nothing WHATEVER ITS COLUMNS HOLD -- NaN, Inf, the
 *   zeros between two packed recordings whose l2-normalised input is 0 / 0: this is a rule about selection, not a product with 0.
 * RESULT: L = sum over the selected (row, e) of w sum_o (y[o] - t[o])^2; Wsum = the sum of the selected w; g = dL / dtheta with
 *   the transfer derivatives TanSig 1 - h^2, LogSig h (1 - h), PureLin 1, SatLin 1 where 0 < a < 1 and else 0; the reverse output
 *   maps are affine (1 / gain); no input function is differentiated, none has a trainable parameter.  d_loss: double [2] =
 *   {L, Wsum}; d_gradient: float [P].  Dividing by Wsum is the caller's.
 * REPRODUCIBLE: the same arrays through the same trainer give the same bits, call after call.  The grid and the order of every sum
 *   are functions of the shapes alone, never of the device or of timing; there are no float atomics.  A row is cut into tiles of
 *   `tile` evaluations (syldet_trainer_shape); workgroup g of G = min(tiles, a bound from P) takes the tiles g, g + G, .. in order,
 *   adds each tile's fp32 sums into its fp64 partial, and a second kernel adds the G partials in order and rounds once to fp32.
 * LIMITS of this version, anything else SYLDET_ERR_UNSUPPORTED at creation: a plain bank (one network: not multi-network, mixed or
 *   sharded; a multi-network bank has syldet_trainer_create_multi below), exactly two layers, H <= SYLDET_TRAIN_MAX_HIDDEN, O <= SYLDET_TRAIN_MAX_OUTPUTS, and an input that fits the
 *   kernel's local memory (290 and 1160 inputs do); any scaling, any input chain, any output chain.
 *   syldet_trainer_create    h: the bank; r: NULL (D = its channels) or a packed-recordings handle of h (D = its recordings).  The
 *       network's fixed part, for recordings the slots, and the partial sums' scratch are put on the device once.  h, and r if
 *       given, must outlive the trainer.
 *   syldet_trainer_shape     D, P, O and the tile (each may be NULL)
 *   syldet_train_param_count host only: P of a configuration of two layers
 *   syldet_train_targets_device   writes EVERY element of d_targets [rows][n_evals][O] and d_weights [rows][n_evals].  For evaluation
 *       e of detector d: target[o] = 1.0 iff some label j of d with label_output[j] == o has |idx_e - t_j| <= half_width_samples,
 *       else 0.0; weight = weight_positive if any target is 1, else weight_negative (either may be 0).  Every (row, e) that belongs
 *       to no detector -- with r: between recordings and behind the last one -- gets target 0 and weight 0.  labels, label_begin
 *       [D + 1] as the scorer's (host arrays; sorted per detector, they may repeat, overlap, lie before 0 or behind the end);
 *       label_output [n_labels] int32 or NULL (all 0).  Integers and two constants only: device, host and any model agree to the
 *       bit (csrc/train_targets.hpp: one text for the kernel, the host and a stand-alone test).  One launch
 *       ("train_targets_kernel").  With r n_evals must be row_evals.
 *   syldet_train_targets_host     host only, one detector in plain C++ (the text the kernel runs): targets [n_evals][n_out],
 *       weights [n_evals].
 *   syldet_train_gradient_device  d_columns [rows][n_frames][bins] as syldet_spectrogram_device wrote it, rows row_stride ELEMENTS
 *       apart (0: n_frames bins); n_evals evaluations a row read n_evals + timeRange - 1 frames (with r: n_evals = row_evals and
 *       n_frames = syldet_count_frames(h, row_samples)); d_params: theta.  Two launches ("train_gradient_kernel",
 *       "train_combine_kernel").  Without a selected evaluation, or with n_evals = 0, L = 0, Wsum = 0 and g = 0 exactly.
 * Statuses, decided before any device is touched; a refused call leaves d_loss and d_gradient as they were.
 * SYLDET_ERR_INVALID_ARGUMENT: a NULL handle or pointer (the device arrays may be NULL where n_evals is 0), a negative n_evals or
 * n_frames, a wrong n_evals or n_frames with r, fewer frames than the evaluations read, a row_stride smaller than a row needs, a
 * label_begin that does not start at 0 or that decreases, unsorted labels, a label_output outside [0, O), a half width outside
 * [0, 2^40], a class weight that is NaN or negative.
 * THE LAUNCH RULE is the aligner's: the trainer keeps the labels on the device.  A targets call whose host arrays differ from the
 * kept ones (the first always) waits for the stream of the trainer's last call and uploads them with one blocking copy; the same
 * arrays again are a launch only.  syldet_train_gradient_device is always launches only: no allocation, no synchronisation, no
 * copy.  One stream at a time, as the bank; every call records into the profile of h (syldet_profile).                         */
#define SYLDET_TRAIN_MAX_HIDDEN  16
#define SYLDET_TRAIN_MAX_OUTPUTS 4
typedef struct syldet_trainer syldet_trainer_t;
int syldet_trainer_create(const syldet_t *h, const syldet_recordings_t *r, syldet_trainer_t **out);
int syldet_trainer_destroy(syldet_trainer_t *t);
int syldet_trainer_shape(const syldet_trainer_t *t, int32_t *n_detectors, int64_t *n_params, int32_t *n_out, int32_t *tile);
int syldet_train_param_count(const syldet_config_t *cfg, int64_t *n_params);
int syldet_train_targets_device(syldet_trainer_t *t, const int64_t *labels, const int64_t *label_begin, const int32_t *label_output,
                                int64_t half_width_samples, float weight_positive, float weight_negative, int64_t n_evals,
                                float *d_targets, float *d_weights, void *hip_stream);
int syldet_train_targets_host(const int64_t *labels, int64_t n_labels, const int32_t *label_output, int32_t n_out,
                              int64_t half_width_samples, float weight_positive, float weight_negative, int64_t first_index,
                              int64_t hop, int64_t n_evals, float *targets, float *weights);
int syldet_train_gradient_device(syldet_trainer_t *t, const float *d_columns, int64_t n_frames, int64_t row_stride,
                                 const float *d_params, const float *d_targets, const float *d_weights, int64_t n_evals,
                                 double *d_loss, float *d_gradient, void *hip_stream);

/* ---- training from the tool: the input map's range, an optimiser, seeded weights and the text writer ----
 * The calls above give loss and gradient; these make the network: the mapminmax that MATLAB refits before it trains (without it the
 * tanh units saturate), the optimiser's step, a fit that is launches only, a seeded start and the writer of the text format -- so
 * that matches -> syldet_train_fit_device -> the scorer needs nothing but this header.  THE CONVENTION is the library's own:
 * THE INPUT RANGE: for every input position i the least and the greatest value the position takes BEHIND THE INPUT FUNCTIONS IN
 *   FRONT OF THE CONFIGURATION'S FIRST mapminmax -- scaling and functions evaluated as the gradient evaluates them, by the same
 *   code -- over the CONTRIBUTING evaluations: those with weight > 0 (a NaN weight does not) whose I values there are all finite.
 *   An evaluation that does not contribute contributes nothing whatever its columns hold (selection, as in the gradient).
 *   d_range: float [2][I] = {least, greatest}, a zero written as +0.0; d_count: int64 [1], the contributing evaluations; with
 *   none, {+inf, -inf} and 0.  The least and the greatest of finite values do not depend on order: the result is a function of
 *   the arrays alone.  A bank without a mapminmax input function: SYLDET_ERR_UNSUPPORTED.
 * THE INPUT MAP of a range: x_offsets = least, gains = fp32(2) / (greatest - least) in fp32, 1 where that difference is not above
 *   0; yMin is -1 (syldet_train_input_map_host).  The trainer keeps ITS OWN COPY of the first mapminmax's parameters on the device:
 *   syldet_trainer_set_input_map replaces them there (the bank and its configuration are not touched), later gradient, range and
 *   fit calls of the trainer use them, syldet_trainer_input_map reads them back (index: the function's place in the chain).
 * ADAM, on the moments m and v (2 P floats) the trainer keeps from creation.  Step number t >= 1; lr, beta1, beta2 and eps are
 *   doubles (the usual defaults: 0.01, 0.9, 0.999, 1e-8).  On the host, in double: c1 = (float)(lr / (1 - pow(beta1, t))),
 *   c2 = (float)(1 / sqrt(1 - pow(beta2, t))).  Per parameter, every operation rounded to fp32 on its own
 *   (csrc/train_adam.hpp: one text for the kernel, the host and a stand-alone test, built without multiply-add contraction):
 *       s = Wsum > 0 ? (float)(1.0 / Wsum) : 0.0f          (Wsum = d_loss[1], read on the device: nothing synchronises)
 *       g = grad * s
 *       m = (float)beta1 * m + (float)(1 - beta1) * g
 *       v = (float)beta2 * v + (float)(1 - beta2) * (g * g)
 *       p = p - c1 * (m / (sqrtf(v) * c2 + (float)eps))
 *   At t = 1 the old m and v are NOT READ and count as 0: a fit needs no memset, and stale or NaN moments cannot leak.  Where Wsum
 *   is not above 0 the parameters keep their bits (the moments follow the lines above with g = 0).  The mean loss written is
 *   L / Wsum in double, 0 where Wsum is not above 0.
 *   syldet_train_input_range_device   rows, detectors, tiles, n_evals, n_frames and row_stride are syldet_train_gradient_device's,
 *       with r and without; so are the statuses.  Two launches ("train_range_kernel", "train_range_combine_kernel"): no
 *       allocation, no synchronisation, no copy, no atomics; the partials lie in the scratch the gradient uses.
 *   syldet_train_input_map_host       host only: range [2][I] -> x_offsets [I], gains [I].
 *   syldet_trainer_set_input_map      waits for the stream of the trainer's last call and makes one blocking copy (the launch
 *       rule of the targets call).  SYLDET_ERR_UNSUPPORTED without a mapminmax input function; a NaN y is refused.
 *   syldet_trainer_input_map          each pointer may be NULL.
 *   syldet_train_adam_device          one step on d_params [P] in place from d_loss [2] and d_gradient [P] as the gradient call
 *       left them; d_mean_loss: double [1] or NULL.  One launch ("train_adam_kernel").
 *   syldet_train_adam_host            host only, the same text: params, m, v [n_params] in place; loss [2]; mean_loss may be NULL.
 *   syldet_train_fit_device           enqueues `steps` x (gradient, combine, step t = 1 .. steps): 3 x steps launches and nothing
 *       else, with the loss and the gradient in the trainer's own scratch.  d_params [P] is updated in place, d_history [steps]
 *       gets the mean loss in front of every step.  Parameters and history after k steps are bit for bit those of k separate
 *       syldet_train_gradient_device + syldet_train_adam_device calls.  Every step is one call of the profile.
 *   syldet_train_init_host            host only, theta [P] for (I, H, O): SplitMix64 from `seed` (state += 0x9E3779B97F4A7C15;
 *       z = state; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31), the k-th draw
 *       u = fp32(z >> 40) * 2^-23 - 1 in [-1, 1), exact; in theta's order W1 = u * fp32(sqrt(3.0 / I)), b1 = u * 0.35f,
 *       W2 = u * fp32(sqrt(3.0 / H)), b2 = 0 without draws.
 *   syldet_train_config_with          a copy of cfg with the two layers' parameters replaced by params [n_params] (n_params must
 *       be P) and, where x_offsets is not NULL, the first mapminmax input function's x_offsets, gains and y; freed by
 *       syldet_config_free.
 *   syldet_config_save_text           writes cfg in the text format syldet_config_load_text reads, numbers as "%.15g" (the
 *       sampling rate and the frequency range as "%.1f"): what convert_to_text.m writes.  SYLDET_ERR_PARSE_OPEN: the file
 *       cannot be written.
 * Statuses, decided before any device is touched; a refused call leaves its results (and d_params) as they were.
 * SYLDET_ERR_INVALID_ARGUMENT: what syldet_train_gradient_device refuses, a step outside [1, 2^31], steps outside [0, 2^31], an
 * lr that is not finite, a beta outside [0, 1), an eps that is negative or not finite, a wrong n_params.                        */
int syldet_train_input_range_device(syldet_trainer_t *t, const float *d_columns, int64_t n_frames, int64_t row_stride,
                                    const float *d_weights, int64_t n_evals, float *d_range, int64_t *d_count, void *hip_stream);
int syldet_train_input_map_host(const float *range, int32_t n_inputs, float *x_offsets, float *gains);
int syldet_trainer_set_input_map(syldet_trainer_t *t, const float *x_offsets, const float *gains, float y);
int syldet_trainer_input_map(const syldet_trainer_t *t, int32_t *index, float *x_offsets, float *gains, float *y);
int syldet_train_adam_device(syldet_trainer_t *t, float *d_params, const double *d_loss, const float *d_gradient, int64_t step,
                             double lr, double beta1, double beta2, double eps, double *d_mean_loss, void *hip_stream);
int syldet_train_adam_host(float *params, float *m, float *v, const float *gradient, int64_t n_params, const double *loss,
                           int64_t step, double lr, double beta1, double beta2, double eps, double *mean_loss);
int syldet_train_fit_device(syldet_trainer_t *t, const float *d_columns, int64_t n_frames, int64_t row_stride,
                            const float *d_targets, const float *d_weights, int64_t n_evals, float *d_params, int64_t steps,
                            double lr, double beta1, double beta2, double eps, double *d_history, void *hip_stream);
int syldet_train_init_host(uint64_t seed, int32_t n_inputs, int32_t n_hidden, int32_t n_outputs, float *theta);
int syldet_train_config_with(const syldet_config_t *cfg, const float *params, int64_t n_params, const float *x_offsets,
                             const float *gains, float y, syldet_config_t **out);
int syldet_config_save_text(const syldet_config_t *cfg, const char *path);

/* ---- training a network per channel: the trainer of a multi-network bank ----
 * A rig with N birds needs N networks, each trained on its own bird's rows.  syldet_trainer_create_multi makes ONE trainer for the N
 * networks of a syldet_create_multi bank: every call below is then one launch (or two, or 3 x steps) for all of them, and network
 * n's results are BIT FOR BIT what a plain trainer (syldet_trainer_create) on a plain bank of network n gives on that network's rows
 * alone.  syldet_trainer_create itself is unchanged: it still refuses multi-network banks.
 * THE CONVENTION:
 *   - Network n's rows are the bank's rows whose channel_net is n, in ascending order.  With r a recording trains the network of
 *     the row it was planned onto.
 *   - Its tiles are those rows' tiles, numbered row-major; its workgroups are G_n = min(tiles_n, the plain trainer's bound for P)
 *     (syldet_trainer_groups).  Workgroup g of network n takes the tiles g, g + G_n, .. in order; its fp64 partial and the combine
 *     in group order are the plain kernel's, from the same text.
 *   - Hence network n's {L, Wsum}, gradient, range, count, Adam step and fit history have THE BITS a plain trainer on a plain bank
 *     of that network gives on those rows alone: the same columns, targets and weights gathered contiguously, with r = NULL.
 *   - A trainer made by syldet_trainer_create_multi always runs the multi form, also at N = 1 (a plain bank).
 *   - A network without a selected evaluation (or without a row) gives L = 0, Wsum = 0 and g = 0 exactly; Adam leaves its
 *     parameters' bits.  Adam's 1 / Wsum is per network; c1 and c2 are shared.
 * Each network's fixed part -- the input functions' x_offsets, gains and y, the output maps -- is read from ITS OWN configuration;
 * compatibility (syldet_config_compatible) guarantees that the shapes, kinds, scaling and transfers are shared.
 * THE ARRAYS of the calls above on such a trainer take a leading network dimension: d_params [N][P], d_loss [N][2], d_gradient
 * [N][P], d_range [N][2][I], d_count [N], d_mean_loss [N], d_history [steps][N]; the moments are [N] x 2 P inside the trainer.
 * Targets, weights and columns stay [rows][n_evals].. and syldet_train_targets_device is unchanged.  Statuses, the launch rule
 * (gradient, range, Adam and fit are launches only: no allocation, no synchronisation, no copy; the group tables go to the device
 * at creation) and the profile's names are the plain trainer's.
 * LIMITS of this version: a plain bank (N = 1) or a syldet_create_multi bank; mixed and sharded banks stay SYLDET_ERR_UNSUPPORTED,
 *   and every limit of the plain trainer holds for each network (two layers, H <= 16, O <= 4, the local memory, <= 8 functions,
 *   N x P <= 2^31 - 1, N <= 65535).  The scratch is N x the plain trainer's, reserved at creation: SYLDET_ERR_OUT_OF_MEMORY where it does
 *   not fit.  Out of scope: the command-line tool (--train keeps taking one network), mixed and sharded banks, a matrix-
 *   instruction form of the first layer's gradient, deeper networks.
 *   syldet_trainer_create_multi   h: a plain bank or a syldet_create_multi bank; r: NULL or a packed-recordings handle of h.
 *   syldet_trainer_networks       N and (may be NULL) row_network [rows]: each bank row's network.  Any trainer (plain: 1, zeros).
 *   syldet_trainer_groups         host only: groups [N] <- G_n for n_evals evaluations a row.  Any trainer.
 *   syldet_trainer_set_input_map_of, syldet_trainer_input_map_of   syldet_trainer_set_input_map and syldet_trainer_input_map (which
 *       address network 0) for network `net`; a net outside [0, N) is SYLDET_ERR_INVALID_ARGUMENT.                              */
int syldet_trainer_create_multi(const syldet_t *h, const syldet_recordings_t *r, syldet_trainer_t **out);
int syldet_trainer_networks(const syldet_trainer_t *t, int32_t *n_networks, int32_t *row_network);
int syldet_trainer_groups(const syldet_trainer_t *t, int64_t n_evals, int32_t *groups);
int syldet_trainer_set_input_map_of(syldet_trainer_t *t, int32_t net, const float *x_offsets, const float *gains, float y);
int syldet_trainer_input_map_of(const syldet_trainer_t *t, int32_t net, int32_t *index, float *x_offsets, float *gains, float *y);

/* ---- template matching: find a syllable's occurrences in the columns ----
 * The scorer, the aligner and the trainer all start from labels; in the workflow the reference belongs to, labels come from matching
 * one exemplar of the syllable against the whole archive.  These calls do that on the columns that lie on the device: exemplar ->
 * matches -> syldet_train_targets_device / the scorer / syldet_align_device.  THE CONVENTION is the library's own:
 * A DETECTOR, its frames u in [0, U_d) and the placement of a packed recording's frames in its row are the aligner's
 *   SYLDET_ALIGN_COLUMNS definitions.  The source is [rows][n_frames][bins] as syldet_spectrogram_device wrote it (linear values),
 *   rows row_stride ELEMENTS apart (0: n_frames bins).
 * THE TEMPLATE is n >= 1 frames of `bins` floats, every value finite, not all zero, n bins <= SYLDET_MATCH_MAX_TEMPLATE; bins must
 *   be the bank's.  At creation the library makes t^ = fp32(t / ||t||_2), the norm and the division in fp64;
 *   syldet_matcher_template returns t^, which is what every model uses.
 * THE SCORE of position p of a detector, 0 <= p <= U_d - n, is the cosine between its window and the template:
 *     s(p) = dot / sqrt(E),   dot = sum_{j < n, b < bins} t^[j][b] x[p + j][b],   E = sum_{j < n, b < bins} x[p + j][b]^2
 *   in fp32; nothing is subtracted.  E == 0 gives +0.0 (silence matches nothing); a window that holds a NaN or an Inf gives NaN, a
 *   window that holds neither the score of its own values; windows whose E would pass 2^100 are outside the contract.
 *   A SCORE IS A FUNCTION OF ITS WINDOW'S VALUES AND t^ ALONE: it has the same bits wherever the window lies in a row, a tile, a
 *   launch or a bank, so a packed recording's scores are its scores through a one-channel handle, bit for bit.  (dot is one chain
 *   of fused multiply-adds a group of 4 bins -- groups g, g + 4, .. of the padded bins together, up to four such chains -- over
 *   the window in (frame, bin) order from +0.0, the chains added in order; E is the sum, from the window's first frame on, of
 *   the frames' energies, each a chain over its bins; frames outside the window only ever meet zeros, and a NaN or an Inf enters
 *   the products as zero and reaches the score through E alone.)
 * THE RESULT is d_scores [rows][n_frames] fp32, every element written exactly once: element first + p of a detector's row is s(p)
 *   (first: 0 for a channel, slot.first_eval for a recording); every other element -- the last n - 1 positions of a detector, frames
 *   between recordings, a row's tail, all positions of a detector shorter than the template -- is NaN.
 * PEAKS.  Given threshold (not NaN; -inf allowed) and separation S (0 <= S <= SYLDET_MATCH_MAX_SEPARATION frames), position p is a
 *   MATCH iff s(p) is not NaN, s(p) >= threshold, s(q) < s(p) for every non-NaN q in [p - S, p) and s(q) <= s(p) for every non-NaN q
 *   in (p, p + S] of the same detector: the earliest position of a tie wins, a NaN neither matches nor suppresses.  A pure function of
 *   the fp32 scores (csrc/match_peaks.hpp: one text for the kernel, the host and a stand-alone test).
 * EVENTS.  A match at p with anchor frame a (0 <= a < n, fixed at creation; negative: n - 1) is the sample number
 *   origin + (p + a) hop with origin and hop of syldet_align_anchor(COLUMNS): its anchor frame under the aligner is p + a, and with
 *   a = n - 1 an aligner of before = n - 1, after = 0 cuts exactly the matched window.  d_events [D][capacity] int64 ascending,
 *   d_counts [D] int64 (may exceed capacity), d_event_scores [D][capacity] fp32 or NULL: the detection calls' tables, which go as
 *   they are into syldet_align_device (event_stride = capacity), the scorer and syldet_train_targets_device.
 *   syldet_matcher_create    h: the bank; r: NULL (D = its channels) or a packed-recordings handle of h (D = its recordings).  t^ and,
 *       for recordings, the slots go to the device once.  h, and r if given, must outlive the matcher.
 *   syldet_matcher_shape     D, n, bins, the anchor, and whether the score kernel takes the matrix form (each may be NULL)
 *   syldet_matcher_template  t^ [n][bins]
 *   syldet_match_scores_device   one launch.  "match_scores_mfma_kernel": a workgroup stages the frames of 256 positions in LDS once
 *       and takes dot on v_mfma_f32_16x16x4_f32 against a Toeplitz operand of the template, the frames' energies from the same
 *       staged values; "match_scores_plain_kernel", one thread a position, where that tile does not fit 64 KB of LDS -- a function
 *       of n and bins alone (29 bins at n = 91 and below take the matrix form).  With r n_frames must be
 *       syldet_count_frames(h, row_samples).
 *   syldet_match_peaks_device    one launch ("match_peaks_kernel": a workgroup a detector; maxima of blocks of 2^k positions, two of
 *       which cover any S, so the work a position grows with log S; a scan places the events in order).
 *   syldet_match_normalize_host  host only: t^ of a template
 *   syldet_match_scores_host     host only, one detector: columns [n_frames][bins] -> scores [n_frames] as THE RESULT has them; fp32
 *       in an order of the library's choice, which need not be the device's
 *   syldet_match_peaks_host      host only, one detector in plain C++ (the text the kernel runs): scores [n_positions] -> events,
 *       *count, event_scores (may be NULL); origin in [0, 2^32), hop in [1, 2^31).
 * Statuses, decided before any device is touched; a refused call leaves its outputs as they were.  SYLDET_ERR_INVALID_ARGUMENT: a
 * NULL handle or pointer (the device arrays may be NULL where n_frames is 0, d_events where capacity is 0), a template outside the
 * rules above, other bins than the bank's, an anchor >= n, a negative n_frames or capacity, a wrong n_frames with r, a row_stride
 * smaller than a row needs, a NaN threshold, a separation outside its range.  SYLDET_ERR_UNSUPPORTED: a mixed bank of more than one
 * class, as syldet_spectrogram* answers there.  A sharded bank has none: the language bindings answer SYLDET_ERR_UNSUPPORTED.
 * THE LAUNCH RULE: the matcher keeps t^ and the slots on the device from creation; both device calls are launches only -- no
 * allocation, no synchronisation, no copy -- and their number does not depend on D.  One stream at a time, as the bank; every call
 * records into the profile of h (syldet_profile) under its kernel's name.                                                        */
#define SYLDET_MATCH_MAX_TEMPLATE   32768
#define SYLDET_MATCH_MAX_SEPARATION 4096
typedef struct syldet_matcher syldet_matcher_t;
int syldet_matcher_create(const syldet_t *h, const syldet_recordings_t *r, const float *templ, int32_t n, int32_t bins, int32_t anchor,
                          syldet_matcher_t **out);
int syldet_matcher_destroy(syldet_matcher_t *m);
int syldet_matcher_shape(const syldet_matcher_t *m, int32_t *n_detectors, int32_t *n, int32_t *bins, int32_t *anchor, int32_t *matrix_form);
int syldet_matcher_template(const syldet_matcher_t *m, float *t_hat);
int syldet_match_scores_device(syldet_matcher_t *m, const float *d_columns, int64_t n_frames, int64_t row_stride, float *d_scores,
                               void *hip_stream);
int syldet_match_peaks_device(syldet_matcher_t *m, const float *d_scores, int64_t n_frames, float threshold, int32_t separation,
                              int64_t *d_events, int64_t capacity, int64_t *d_counts, float *d_event_scores, void *hip_stream);
int syldet_match_normalize_host(const float *templ, int32_t n, int32_t bins, float *t_hat);
int syldet_match_scores_host(const float *t_hat, int32_t n, int32_t bins, const float *columns, int64_t n_frames, float *scores);
int syldet_match_peaks_host(const float *scores, int64_t n_positions, float threshold, int32_t separation, int64_t origin, int64_t hop,
                            int32_t anchor, int64_t *events, int64_t capacity, int64_t *count, float *event_scores);

/* ---- template matching: a bank of templates ----
 * A real song has several syllable types, and one exemplar of a syllable is a poor detector of it: a lab keeps a handful of
 * exemplars a syllable and takes the best of them.  A bank does that in one pass over the columns: the frames of a tile are staged
 * and their energies taken once for all templates, where K matchers pay both K times.  Everything the section above defines -- the
 * detector, the template's rules and t^, the score, the result's NaN, the peaks rule, the events -- holds here for every template.
 * A BANK is K templates, 1 <= K <= SYLDET_MATCH_MAX_TEMPLATES, each [n][bins]; all share one n, one bins and one anchor; each obeys
 *   the single template's rules (finite, not all zero, n bins <= SYLDET_MATCH_MAX_TEMPLATE) and is normalised on its own as
 *   syldet_match_normalize_host does it.
 * CLASSES.  template_class[k] lies in [0, C), 1 <= C <= SYLDET_MATCH_MAX_CLASSES; every class has at least one template.  A class
 *   is a syllable, its templates that syllable's exemplars.  A NULL template_class means class k = k and C = K (n_classes K or 0),
 *   which is refused when K > SYLDET_MATCH_MAX_CLASSES.
 * THE TEMPLATE SCORE s_k(p) is the single matcher's score of template k at position p WITH THE SAME BITS: the same chains in the
 *   same order in the same form.  The form (matrix or plain) is the single matcher's function of (n, bins); K does not enter it.
 * THE CLASS SCORE S_c(p) is the greatest s_k(p) over the templates of class c.  All templates share n, so they share windows: a
 *   position is NaN for every template or for none, and its NaN-ness, its E and its +0.0 on silence are the single matcher's.  The
 *   templates are taken in ascending k and the running value is replaced only where s_k > running, so which_c(p) is the LOWEST k
 *   of the class that attains the maximum; it is -1 where the score is NaN.  Comparisons only: S_c(p) has the bits of
 *   s_{which_c(p)}(p).  (csrc/match_classes.hpp: one text for the kernels, the host and a stand-alone test.)
 * THE RESULT is d_scores [C][rows][n_frames] fp32, every element written exactly once, NaN wherever the single matcher writes NaN;
 *   d_which [C][rows][n_frames] int32 or NULL, every element written exactly once when given.
 * PEAKS.  Each class is matched on its own plane by the rule above (csrc/match_peaks.hpp, unchanged) with its own thresholds[c]
 *   -- a HOST array of C floats, none NaN, passed to the kernel by value: nothing is uploaded -- and the shared separation.
 *   d_events [C][D][capacity], d_counts [C][D], d_event_scores [C][D][capacity] or NULL; d_event_template [C][D][capacity] int32 or
 *   NULL is which at each matched position and needs d_which (SYLDET_ERR_INVALID_ARGUMENT without it).  Class c's tables are byte
 *   for byte what syldet_match_peaks_device writes from plane c with thresholds[c].  CLASSES DO NOT SUPPRESS EACH OTHER: two
 *   classes may match at the same position, and a caller who wants one label a position decides between them.
 *   syldet_matcher_bank_create     h, r, the anchor as syldet_matcher_create; templates [K][n][bins].  The normalised templates,
 *       the class table and, for recordings, the slots go to the device once.
 *   syldet_matcher_bank_shape      D, K, C, n, bins, the anchor, the form (each may be NULL)
 *   syldet_matcher_bank_templates  t^ [K][n][bins] and the class of each template (either may be NULL)
 *   syldet_match_bank_scores_device   ONE launch for any K and C.  "match_bank_scores_mfma_kernel" keeps the tile, the grid and the
 *       LDS layout of "match_scores_mfma_kernel": the frames of 256 positions are staged once, their energies taken and the
 *       non-finite values zeroed once, E of a position summed once; every template then makes one pass of the same
 *       v_mfma_f32_16x16x4_f32 chain over the staged frames through the one template region of the tile, the next template staged
 *       behind the barrier that ends a pass.  "match_bank_scores_plain_kernel" where the single matcher takes the plain form.
 *   syldet_match_bank_peaks_device    ONE launch for any C and D ("match_bank_peaks_kernel", grid (D, C): the body of
 *       "match_peaks_kernel" a class).
 *   syldet_match_classes_host      host only: template scores [K][n_positions] -> class_scores [C][n_positions] and which (may be
 *       NULL) by the rule above; of the values given, a NaN is never taken, so a position is NaN, -1 iff all its class's are NaN.
 * Statuses as above, decided before any device is touched; besides: K or C outside their ranges, a class outside [0, C), a class
 * without a template, NULL thresholds or a NaN among them, d_event_template without d_which are SYLDET_ERR_INVALID_ARGUMENT.  Mixed
 * and sharded banks get the answers the single matcher gives them.
 * THE LAUNCH RULE is the matcher's: both device calls are launches only -- no allocation, no synchronisation, no copy -- and each
 * records into the profile of h under its kernel's name.
 * NOT HERE: suppression across classes; a class column in label files; training more than output 0 from the command-line tool;
 * sharded banks.  (Templates of their own lengths: the next section.)                                                            */
#define SYLDET_MATCH_MAX_TEMPLATES 64
#define SYLDET_MATCH_MAX_CLASSES   16
typedef struct syldet_matcher_bank syldet_matcher_bank_t;
int syldet_matcher_bank_create(const syldet_t *h, const syldet_recordings_t *r, const float *templates, int32_t n_templates, int32_t n,
                               int32_t bins, int32_t anchor, const int32_t *template_class, int32_t n_classes, syldet_matcher_bank_t **out);
int syldet_matcher_bank_destroy(syldet_matcher_bank_t *m);
int syldet_matcher_bank_shape(const syldet_matcher_bank_t *m, int32_t *n_detectors, int32_t *n_templates, int32_t *n_classes, int32_t *n,
                              int32_t *bins, int32_t *anchor, int32_t *matrix_form);
int syldet_matcher_bank_templates(const syldet_matcher_bank_t *m, float *t_hat, int32_t *template_class);
int syldet_match_bank_scores_device(syldet_matcher_bank_t *m, const float *d_columns, int64_t n_frames, int64_t row_stride, float *d_scores,
                                    int32_t *d_which, void *hip_stream);
int syldet_match_bank_peaks_device(syldet_matcher_bank_t *m, const float *d_scores, const int32_t *d_which, int64_t n_frames,
                                   const float *thresholds, int32_t separation, int64_t *d_events, int64_t capacity, int64_t *d_counts,
                                   float *d_event_scores, int32_t *d_event_template, void *hip_stream);
int syldet_match_classes_host(const float *template_scores, int64_t n_positions, int32_t n_templates, const int32_t *template_class,
                              int32_t n_classes, float *class_scores, int32_t *which);

/* ---- template matching: a ragged bank ----
 * The syllables of one song do not share a duration, and exemplars of one syllable cut from different renditions differ by a frame
 * or two.  A ragged bank holds templates of different lengths in one bank, so the frames are staged and their energies taken once
 * for all of them; with different lengths "position = first frame of the window" no longer lines the templates of a class up, so
 * THE TEMPLATES ARE LINED UP AT THEIR ANCHORS.  The handle is the bank's (syldet_matcher_bank_t); everything the two sections above
 * define holds for every template.  A bank made by syldet_matcher_bank_create is untouched: its kernels, its planes (indexed by the
 * window's first frame) and its bytes stay as they are.
 * A RAGGED BANK is K templates, 1 <= K <= SYLDET_MATCH_MAX_TEMPLATES; template k is [n_k][bins], n_k >= 1, n_k bins <=
 *   SYLDET_MATCH_MAX_TEMPLATE; `templates` is their concatenation in k order; each obeys the single template's rules and is
 *   normalised on its own as syldet_match_normalize_host does it.  template_n[k] = n_k.  template_anchor[k] = a_k lies in [0, n_k); a
 *   NULL table means n_k - 1 for every k.  Classes are the bank's: the same table rules, NULL = identity, C <=
 *   SYLDET_MATCH_MAX_CLASSES.
 * THE PLANES ARE INDEXED BY THE ANCHOR FRAME.  Element first + u of a detector's row in plane c belongs to frame u of the detector,
 *   0 <= u < U_d.  Template k's window for u is the frames [u - a_k, u - a_k + n_k); it exists iff 0 <= u - a_k and
 *   u - a_k + n_k <= U_d: it lies inside the detector's own frames ON BOTH SIDES.  The front side is new: a packed recording's window
 *   never reads the previous recording of its row or the gap before it.  Where the window exists, s_k(u) is the single matcher's
 *   score of template k on that window.
 * THE CLASS SCORE S_c(u) is the greatest s_k(u) over the templates of class c whose window exists at u and whose score is not NaN,
 *   taken in ascending k and replaced only where greater (csrc/match_classes.hpp: a NaN is never taken); which is the LOWEST k that
 *   attains it; the result is NaN, -1 iff no template of the class has a non-NaN score there.  Unlike the uniform bank a position can
 *   be NaN for one template and not for another: near a detector's ends the shorter window fits where the longer does not, and the
 *   shorter window can miss a NaN or an Inf that the longer one holds.
 * BITS.  The bank's form is matrix iff its tile (below) fits the single matcher's 64 KB; otherwise every template takes the plain
 *   form.  In a matrix-form bank every template's single matcher is matrix-form too (its tile is no larger), so s_k(u) has the bytes
 *   of syldet_matcher_create(template k)'s score at position u - a_k: the chains, their order, the zeros by selection, E as the chain
 *   of frame energies from the window's first frame on and the division are the same device functions.  In a plain-form bank s_k
 *   has the plain form's bytes, which are the single matcher's wherever the single matcher of (n_k, bins) is plain as well; where it
 *   is not -- a 12-frame template beside a 100-frame one at 29 bins -- the score is the plain form's of the same sums, within the
 *   single matcher's distance of the fp64 value.
 * EVENTS.  A match at u is the sample origin + u hop: the plane's index is the anchor, so the plane's own anchor is 0.  The peaks
 *   rule is csrc/match_peaks.hpp, unchanged, over all U_d elements of the detector; NaN neither matches nor suppresses.  The tables
 *   go as they are into the aligner, the scorer and syldet_train_targets_device.
 * A SEPARATION A CLASS.  A short syllable repeats faster than a long one: syldet_match_bank_peaks_each_device takes `separations`, a
 *   HOST array of C values in [0, SYLDET_MATCH_MAX_SEPARATION] passed by value like the thresholds.  Class c's tables are byte for
 *   byte what syldet_match_peaks_host writes from that detector's stretch of plane c with thresholds[c], separations[c] and (on a
 *   ragged bank) anchor 0.
 *   syldet_matcher_bank_create_ragged   the lengths, anchors, offsets, the class order and, for recordings, the slots go to the device
 *       once.  On its handle syldet_matcher_bank_shape reports the greatest n_k as n and 0 as the anchor, and
 *       syldet_matcher_bank_templates writes the concatenated t^.
 *   syldet_matcher_bank_lengths         n_k and a_k of every template and whether the bank is ragged (each may be NULL); a uniform
 *       bank: K times (n, anchor), 0.
 *   syldet_match_bank_scores_device     on a ragged handle ONE launch for any K, C and lengths.  "match_ragged_scores_mfma_kernel"
 *       keeps the bank kernel's workgroup and its tile of 256 plane elements p0 .. p0 + 255.  With the lead a_max = max a_k and the
 *       tail r_max = max (n_k - a_k) it stages the G = 255 + a_max + r_max frames p0 - a_max .. p0 + 255 + r_max - 1 once (frames
 *       before the row's start and behind its end zero by selection), takes their energies and zeroes the non-finite values once,
 *       and makes one pass a template in the class order through the one template region of n_max frames; template k's pass runs the
 *       bank's products with n_k as loop and selection bound from s_k = a_max - a_k frames into the staged block, and its E from the
 *       same frame.  The tile's floats are counted as the single matcher's with this G and this region (csrc/match_ragged.hpp: one
 *       text for the kernels, the host and a stand-alone test).  "match_ragged_scores_plain_kernel", a thread a plane element, where
 *       that tile does not fit.
 *   syldet_match_bank_peaks_device      works on a ragged handle too (the shared separation).
 *   syldet_match_bank_peaks_each_device ONE launch ("match_bank_peaks_each_kernel": the body of "match_peaks_kernel" a class with the
 *       class's own separation; LDS by the greatest).  On a uniform handle with equal separations it writes the bytes of
 *       syldet_match_bank_peaks_device.
 * Statuses as above, decided before any device is touched; a refused call leaves its outputs as they were.  Besides the bank's:
 * NULL template_n, an n_k < 1 or n_k bins over the limit, an anchor outside [0, n_k), NULL separations or one outside its range are
 * SYLDET_ERR_INVALID_ARGUMENT.  Mixed and sharded banks get the answers the bank gives them.
 * THE LAUNCH RULE is the bank's: no call allocates, synchronises or copies.
 * NOT HERE: exemplars of different lengths within one .npy file of the command-line tool (a file is [k][n][bins]: give one file a
 * length, or use the library); suppression across classes; a class column in label files; sharded banks.                          */
int syldet_matcher_bank_create_ragged(const syldet_t *h, const syldet_recordings_t *r, const float *templates, int32_t n_templates,
                                      const int32_t *template_n, int32_t bins, const int32_t *template_anchor,
                                      const int32_t *template_class, int32_t n_classes, syldet_matcher_bank_t **out);
int syldet_matcher_bank_lengths(const syldet_matcher_bank_t *m, int32_t *template_n, int32_t *template_anchor, int32_t *ragged);
int syldet_match_bank_peaks_each_device(syldet_matcher_bank_t *m, const float *d_scores, const int32_t *d_which, int64_t n_frames,
                                        const float *thresholds, const int32_t *separations, int64_t *d_events, int64_t capacity,
                                        int64_t *d_counts, float *d_event_scores, int32_t *d_event_template, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SYLDET_H */
