// kernels.hpp -- device-side descriptors and launcher prototypes shared by the engine
// files.  Everything here is gfx950-only HIP.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "detector_spans.hpp"

namespace sd {

constexpr int kMaxFns = 8;
constexpr int kMaxLayers = 8;

// STFT geometry + tables (built once per handle by syldet_create).
struct StftDesc {
    int N, W, M, logM;        // fourierLength, windowLength, N/2, log2(N/2)
    int hop, gap;             // frame j covers samples [j*hop + gap, j*hop + gap + W)
    int f0, F;                // band [f0, f0+F)
    int power_mode;           // 0: |X| (extractPower), 1: |X|^2 (extractMagnitude)
    const float *window;      // [W]
    const float2 *tw;         // [M/2]  e^{-2 pi i t / M}     (complex FFT stage twiddles)
    const float2 *sw;         // [M]    e^{-2 pi i k / N}     (real-split twiddles)
    // mixed banks (syldet_create_mixed): channel c of the launch reads samples row row_of[c] of the bank; the columns stay
    // [C][J][F] in launch order.  Null: row c.
    const int *row_of;
};

struct DevFn {
    int kind;                 // syldet_fn_kind_t
    int xoff, gain;           // offsets (in floats) into the parameter blob
    float y;
    int yoff;                 // ... and of y (what a multi-network handle reads: each network has its own y)
};
struct DevLayer {
    int in, out, tf;          // tf: syldet_transfer_t
    int w, b;                 // offsets into the parameter blob; w is row-major [out][in]
};
// The network exactly as configured (generic engine: no algebraic folding).
struct NetDesc {
    int n_in_fns, n_layers, n_out_fns;
    DevFn in_fns[kMaxFns];
    DevLayer layers[kMaxLayers];
    DevFn out_fns[kMaxFns];
    int I, n_out, max_width;
    int scaling;              // syldet_scaling_t
    int rule;                 // syldet_rule_t
    const float *params;      // parameter blob
    const double *thresholds; // [n_out]
    // multi-network handles (syldet_create_multi): channel c reads the blob and thresholds of network net_of[c], which sit
    // params_stride floats / thr_stride doubles apart (compatible networks have the same offsets); null for one network
    const int *net_of;
    int params_stride, thr_stride;
    // mixed banks (syldet_create_mixed): channel c of the launch writes outputs and flags row row_of[c] of the bank (and the
    // exact recomputation reads that samples row); its network stays net_of[c].  Null: row c.
    const int *row_of;
};

// The bank row of a launch's channel c (a mixed bank's class launches: row_of, a uniform load), else c itself.
__device__ __forceinline__ int bank_row(const int *row_of, int c)
{
    return row_of ? __builtin_amdgcn_readfirstlane(row_of[c]) : c;
}

// ---- generic engine (any power-of-two N, any processing chain, any layer sizes) ----
// columns [C][J][F] <- samples [C][stride]
hipError_t launch_stft_generic(const StftDesc &d, const float *samples, int64_t stride, int C, int64_t J,
                               float *columns, hipStream_t stream);
// the same for 128-, 256- and 512-point frames, butterflies across the lanes (kernels_stft_lanes.hip)
bool stft_lanes_applicable(const StftDesc &d, const float *samples, int64_t stride);
hipError_t launch_stft_lanes(const StftDesc &d, const float *samples, int64_t stride, int C, int64_t J, float *columns, hipStream_t stream);
// outputs [C][E][n_out], flags [C][E] <- columns [C][J][F]; either output may be null
hipError_t launch_mlp_generic(const NetDesc &n, int F, const float *columns, int C, int64_t J, int64_t E,
                              float *outputs, uint8_t *flags, hipStream_t stream);
// indices [C][capacity], counts [C] <- flags [C][E]
hipError_t launch_detections(const uint8_t *flags, int C, int64_t E, int64_t first_index, int64_t hop,
                             int64_t debounce_frames, int64_t *indices, int64_t capacity, int64_t *counts,
                             hipStream_t stream);

// ---- wide-network engine (kernels_wide.hip): first layer as a bf16 MFMA GEMM over many evaluations ----
constexpr int kWideBlock = 1024;           // 16 waves, 32 evaluations each
constexpr int kWideTile = 512;             // evaluations per workgroup
constexpr int kWideK = 320;                // inputs per evaluation, zero padded (20 k-steps of 16)
constexpr int kWideChunkBytes = 20 * 64 * 16 + (32 + 4 * 32) * 4;   // 32 hidden units: A fragments, then b0[32], w1[4][32]

struct WideDesc {
    int H, n_chunks;            // first-layer outputs, chunks of 32 of them (zero padded)
    int n_out, tf0, tf1, rule, n_out_fns;
    int sig;                    // TanSig / LogSig hidden layer folded into the tables (see wide_gemm_kernel)
    int m32;                    // the staggered two-workgroup GEMM on v_mfma_f32_32x32x16_bf16, chunks packed for it: SYLDET_WIDE_M32 (kernels_wide.hip, wide_gemm32s_kernel)
    int poly;                   // (sig, shape16) the folded tables are for tanh_poly(acc) instead of 1 / (2^acc + 1): SYLDET_WIDE_TANH_POLY
    int shape16;                // the chunks are packed for v_mfma_f32_16x16x32_bf16 ([k-step of 32][unit tile of 16]): wide_gemm16_kernel
    // front = 1: the GEMM kernel reads the |X| columns itself (an evaluation's inputs are I consecutive floats of [C][J][F]) --
    // the input chain is [l2normalize,] affine maps on linear columns, the affine part folded into the first layer by the host,
    // so the B operands are bf16(v / |v|) (l2 = 1) or bf16(v): no [evaluations][320] image in HBM, no preparation kernel
    int front, l2, I, F;
    int wg8;                    // two workgroups of 8 waves a CU instead of one of 16 (kernels_wide.hip, NWV)
    int stagger;                // (wg8) waves 4-7 run one epilogue behind waves 0-3 (kernels_wide.hip, STG)
    int dma_builtin;            // (wg8, unstaggered) the weight DMA through __builtin_amdgcn_global_load_lds instead of the assembly statement
    int tiles4;                 // (wg8, staggered) one workgroup of 8 waves a CU with four evaluation tiles a wave (kernels_wide.hip, TPW)
    const uint4 *wpack;         // [n_chunks][kWideChunkBytes / 16]
    const float *b1;            // [n_out]
    const float *out_params;    // per output fn: y, gain[n_out], xoff[n_out]
    const double *thresholds;   // [n_out]
};
// columns [C][J][F] -> xn [C*E][kWideK] bf16 (scaling + input functions applied)
int wide_front_stage_floats(int F, int I);
bool wide_front_fits(int F, int I);        // WideDesc::front needs the columns under 512 evaluations in LDS
bool wide_front_fits_half(int F, int I);   // ... and the two-workgroup forms (WideDesc::m32 among them) those under 256 in half a CU's
bool wide_prep_is_chain(const NetDesc &n);   // which of the two preparation kernels launch_wide_prep picks (for timing labels)
hipError_t launch_wide_prep(const NetDesc &n, int F, const float *columns, int C, int64_t J, int64_t E, void *xn, hipStream_t stream);
// xn [NE][kWideK] -> outputs [NE][n_out], flags [NE]
// (front: columns [C][J][F], E evaluations per channel, NE = C E; xn unused)
hipError_t launch_wide_gemm(const WideDesc &d, const void *xn, const float *columns, int64_t J, int64_t E, int64_t NE, float *outputs,
                            uint8_t *flags, hipStream_t stream);

// ---- fused engine (kernels_fused.hip) ----------------------------------------------------
// One kernel: samples -> outputs + flags.  The band-limited windowed DFT of 32 frames at a
// time is a GEMM on the matrix cores (f16 hi/lo split operands, fp32 accumulate), the first
// network layer is folded into a second MFMA on the accumulator tile, the sliding window is a
// diagonal sum over an LDS ring.  Built by make_fused_plan() when the configuration fits.
constexpr int kFusedBlock = 512;        // 8 waves
constexpr int kFusedChunkFrames = 64;   // frames per team chunk (4 waves x 16); a workgroup = 2 teams
constexpr int kFusedTileFrames = 128;   // frames per workgroup period (two chunks)
constexpr int kFusedMaxLoads = 10;      // float4 loads per thread per pass
constexpr int kFusedRBlock = 256;       // register-resident-basis kernel (kernels_fused_r.hip): 4 waves, one per SIMD
constexpr int kFusedRTileFrames = 64;   //   16 frames per wave and pass
constexpr int kFusedRMaxLoads = 10;     //   float4 loads per thread per pass
constexpr int kFusedRPRows = 11 + 3 * 64 + 2;   //   rows of its tap-product ring in LDS (52 floats each)
constexpr int kFusedSBlock = 512;       // symmetric-fold kernel (kernels_fused_s.hip): 8 waves, two per SIMD, each a stream of its own
constexpr int kFusedSTileFrames = 16;   //   frames per wave and tile
constexpr int kFusedColStride = 40;     // halves per column row in LDS: 32 bins + 8 of padding (80 B rows: 16-byte
                                        // aligned, and 16 consecutive rows cover all 64 banks once for ds_read_b128)

// ---- precision guard + exact recomputation (kernels_fixup.hip) ----------------------------
// The fused kernels are block floating point: a pass (64 or 128 frames) is scaled by its loudest sample and split into
// f16 hi + lo.  A window that sits far below that level (a quiet stretch next to a click), a pass with an infinite sample
// or a level step of hundreds of dB cannot be held on that grid.  The kernels know: an evaluation whose window norm,
// measured on the grid it was computed on, is too close to the grid's floor for the network's sensitivity (a host-side
// Lipschitz bound) is reported in a work list, and fixup_kernel recomputes exactly those evaluations from the samples
// (fp64 DFT by definition, the network unfolded in the reference's operation order) behind the fused kernel on the same
// stream.  NaN may then appear only where the reference's windows contain the offending sample.
struct FixItem {
    int c;                      // channel
    unsigned first;             // first evaluation (kind 0) / frame (kind 1: spectrogram columns)
    int count;
    int kind;
};
struct FixList {
    unsigned *counters;         // [0] items appended, [1] workgroups done, [2] items of the last launch, [3] overflow (sticky), [4] the launch's first 10 ns tick (of 8 words)
    FixItem *items;
    unsigned capacity;
    unsigned *host_count = nullptr;   // two page-locked words for the launch's item count and its duration in 10 ns ticks (profiling: syldet_timings), or null
};

struct FusedDesc {
    int W, KS;                  // window length, k-steps of 32 samples (KS*32 >= W)
    int hop, gap, F, T;         // frame advance, leading gap, bins, timeRange
    int H;                      // first-layer outputs
    int norm;                   // 0 none, 1 l2normalize, 2 normalize, 3 normalizestd (first input fn)
    int scaling;
    int n_layers, n_out, tf0, tf1, rule, n_out_fns;
    int I;                      // F*T
    int nsmp, nload;            // samples staged per pass, float4 loads per thread
    int skew;                   // floats of padding after every `hop` staged samples (bank spreading)
    unsigned hop_magic;         // ceil(2^32 / hop): i / hop == umulhi(i, hop_magic) for i < 2^16
    int runs, seg_evals;        // passes per workgroup, evaluations per workgroup segment
    int ps;                     // column slots: 2 (T - 1) for the transition strip + 128 for the pass
    int smp_stride;             // halves between the hi and the lo array of the staged samples
    int col_shift;              // |X| columns are stored as |X| * 2^(cse - col_shift) (2x for |X|^2)
    float w_unscale;            // 1 / (power-of-two scale of the folded first-layer weights)
    int lds_dfrag, lds_smp, lds_colh, lds_coll, lds_stat, lds_red, lds_cst, lds_total;   // byte offsets
    // layout of the register-resident-basis kernel (64-frame passes, staged samples double-buffered, no basis in LDS);
    // r_ok = 0 when the shape does not fit it (long hops)
    int classic_ok;             // the 8-wave kernel's LDS layout fits (else only the register-resident-basis kernel can run the plan)
    int r_ok, r_nsmp, r_nload, r_ps, r_smp_stride, r_runs, r_seg_evals;
    int r_lds_smp, r_lds_p, r_lds_red, r_lds_cst, r_lds_total;   // second sample buffer: r_lds_smp + 4 r_smp_stride
    // layout of the symmetric-fold kernel (kernels_fused_s.hip): per wave a ring of s_ring_chunks x 256 samples + a mirror chunk,
    // rows of s_pstride floats of tap products (4 s_tp products, the frame's sum of squares, its floor weight); s_ok = 0 when the
    // shape does not fit it
    int s_ok, s_waves, s_perm, s_ring_chunks, s_pstride, s_tp, s_lds_wave, s_seg_evals;
    int s_padp;                 // 0, or the padding period (floats) of the fold kernel's sample ring: hops that are multiples of 64 (fused_plan.cpp)
    // ... and its second-fold instantiation (W == N == 256, one quad of units, plain ring): s2_ok; s2_pe / s2_po = band index of
    // the first even / odd bin (0 and 1 in some order): lane group g of a result holds band bins 8 g + s2_pe + 2 i (even tile
    // rows 4 g + i) and 8 g + s2_po + 2 i (odd tile)
    int s2_ok, s2_pe, s2_po;
    int s2_nt;                  // row tiles per parity of the twice-folded form: 1 (up to 32 bins) or 2 (33 .. 64 bins: 4 waves a workgroup)
    int s_cs8, s_cs8_rc;        // hop 128 under a 256-sample window, one quad of units: the ring as whole chunks staggered over the banks (kernels_fused_s.hip, CS8) and its slots
    int no_cs8;                 // the handle was created under SYLDET_FUSED_PAD128=1: the padded pieces where both take the shape (A/B runs)
    int no_fold2;               // the handle was created under SYLDET_FUSED_NOFOLD2=1: the once-folded form where both take the shape (A/B runs)
    const uint4 *sfrag2;        // [2 k-steps][Re even, Re odd, Im even, Im odd][hi,lo][64 lanes] A-operand fragments of the twice-folded basis
    const float *swin2;         // [4 lane groups][2 k-steps][8][2] window coefficients w[128 + m], w[m] for m = 32 ks + 8 g + i
    const float *s2c;           // [64 lanes][8]: cos(pi k / 2) 2^13 for the lane's four even bins, w[192], padding
    const uint4 *afrag_t2;      // afrag_t in the bin order of the twice-folded result
    const uint4 *afrag_w2;      // afrag_w in that order (5 .. 16 hidden units)
    const uint4 *sfrag;         // [W/64 k-steps][s, d][bins 0-15, 16-31][hi,lo][64 lanes] A-operand fragments of the folded basis
    const uint4 *afrag_w;       // [3][HQ quads of hidden units][hi,lo][64 lanes] the first layer with all taps as rows for 5 .. 16 units
    const float *slone;         // [64 lanes][8] the frame's first sample's real coefficients for the lane's bins
    const uint4 *dfrag;         // [KS][re 0-15, re 16-31, im 0-15, im 16-31][hi,lo][64 lanes] A-operand fragments of the DFT basis
    const uint4 *afrag;         // [T][hi,lo][64 lanes] A-operand fragments of the folded first layer (16x16x32)
    const uint4 *afrag_t;       // [3 row tiles][hi,lo][64 lanes] the same layer with all taps as rows (row 4 t + h), K in the
                                // bin order of a magnitude result: k = 8 g + j -> bin 4 g + j (j < 4), 16 + 4 g + j - 4 (j >= 4);
                                // null unless H <= 4
    const int *koff;            // [KS][4] staged-sample offset of k-step ks for lane group g4 (skew applied)
    const float *bias0;         // [H]  b0 + W0 . (constant part of the input maps)
    const float *rvec;          // [H]  (W0 o a) . 1
    const float *w1, *b1;       // layer 1, row-major [n_out][H] (2-layer nets)
    const float *out_params;    // per output fn: y, gain[n_out], xoff[n_out]; behind a lone output fn, for the fold kernel: rcp[n_out], 1 / gain
                                // where that is exact, else 0 (fused_plan.cpp, exact_reciprocal.hpp)
    const double *thresholds;   // [n_out]
    float *spect_out;           // spectrogram instantiation only: [C][J][F] columns
    int spect_power;            //   0: |X|, 1: |X|^2
    // precision guard (see FixItem): thresholds on the window statistic in grid units, from fused_plan.cpp
    float guard_r;              // register-resident-basis kernel: window sum of squares, times 4^(se_ref - se_min)
    float guard_c;              // 8-wave kernel, l2normalize / no normaliser: window sum of squares
    float guard_c_range;        //   normalize: window range;  normalizestd: window sigma
    float guard_range_r;        // symmetric-fold kernel, normalize: window range; normalizestd: window sigma (relative to the loudest frame's floor)
    float guard_rel_r, guard_rel_c;   // no normaliser: the per-column relative criterion (smallest column sum of squares of the
                                      // window) that joins the absolute one
    int guard_se_abs_r, guard_se_abs_c;   // no normaliser: passes scaled below this exponent are loud enough for the floor to matter
    float guard_spect;          // spectrogram instantiation: a frame's column sum of squares (grid units) ...
    int guard_se_abs_s;         //   ... in passes scaled below this exponent
    float guard_loud;           // no normaliser: (window sum of squares in true units) * guard_loud > 1 means the three-product arithmetic's
                                //   2^-21.4 of the column level, through the network, is expected beyond a quarter of the 1e-5 bar (symmetric-fold kernel)
    FixList fix;                // work list of evaluations to recompute (null counters: guard off)
    int force_classic;          // the handle was created under SYLDET_FUSED_CLASSIC=1: the 8-wave kernel where both take the shape
    int no_fold;                // the handle was created under SYLDET_FUSED_NOFOLD=1: not the symmetric-fold kernel
    int ko;                     // diagnostic build only: knock-out mask (SYLDET_FUSED_KO)
    short s_hopk_rc;            // hop 132 under a 256-sample window, one quad of units, the plain ring: the slots of the ring whose schedule is compiled in
                                // (kernels_fused_s.hip, HOP; hopk_schedule.hpp), or 0 -- the shape has no such form, or the handle was created under
                                // SYLDET_FUSED_HOPK=0 (A/B runs).  The launcher's alone; it sits in the padding in front of `stamps`: the kernels' arguments stay where they were.
    signed char s_pairstep;     // the HOP form keeps the two waves of a SIMD in step (pair_progress.hpp): 1, or 0 -- the handle was created under
                                // SYLDET_FUSED_PAIRSTEP=0 (A/B runs).  Read by the HOP instantiations alone.  It shares s_hopk_rc's word (there is no
                                // padding left in front of `stamps`), so the kernels' arguments stay where they were.
    signed char s_out_rcp;      // the lean form's output gain is a power of two whose reciprocal is exact (exact_reciprocal.hpp): 1, and out_params
                                // holds 1 / gain behind the output map; else 0. The launcher's alone (it picks the HOP instantiation that
                                // multiplies instead of dividing: the same bits); the upper byte of what was s_pairstep's short.
    unsigned long long *stamps; // diagnostic build only: [workgroups][16] phase cycle sums (the fold kernel: 16 sums, then a record a wave), else null
};
// What the fold kernel reads of ONE network, for multi-network handles (syldet_create_multi): everything else of FusedDesc is
// the shape, which compatible networks share.  A workgroup reads nets[net_of[its channel]] once, before its tiles.
struct FusedNet {
    const uint4 *afrag_t, *afrag_w, *afrag_t2, *afrag_w2;   // as in FusedDesc
    const float *bias0, *rvec, *w1, *b1, *out_params;
    const double *thresholds;
    float w_unscale, guard_r, guard_rel_r, guard_range_r, guard_loud;
    int guard_se_abs_r;
};
struct FusedMulti {             // (host side: what launch_fused hands the fold kernel's multi-network form)
    const FusedNet *nets;       // [networks]
    const int *net_of;          // [C]
    const int *row_of;          // [C] the bank row of each launch channel (a mixed bank's class launch), or null: row c
};

// ---- first layer on the matrix cores for spectrograms already in HBM (kernels_mlpx.hip) --------------------
// The generic engine's network stage for the detector class the training script writes (l2normalize first, affine
// maps, TanSig hidden layer of at most 4 units, one linear output, at most one output map, linear |X| columns) when the
// band is too wide or the window too long for the fused engine (BASELINE configs[2]: 116 bins of 1024-point frames):
// the fused engine's shifted GEMM over f16 hi/lo columns, fed from [C][J][F] columns instead of from its own DFT.
constexpr int kMlpxBlock = 512;          // 8 waves, 16 frames each
constexpr int kMlpxTile = 128;           // frames per tile (its windows: 128 - timeRange + 1 evaluations)
struct MlpxDesc {
    int F, T, KB, H;            // bins, timeRange, 32-bin blocks per tap (F <= 32 KB), hidden units
    int rule;
    int scaling;                // SYLDET_SCALING_*: linear, ln x or 20 log10 x of the columns in front of the chain (SyllableDetector.swift:184-212)
    int col_stride;             // halves per column row in LDS: 32 KB + 8
    int p_stride;               // floats per frame row of tap products in LDS
    float w_unscale, b1, oa, og, ob;   // 1 / scale of the folded weights; second layer bias; output map (y - oa) / og + ob
    int lds_afrag, lds_colh, lds_coll, lds_p, lds_pq, lds_ss, lds_red, lds_total;   // byte offsets
    const uint4 *afrag;         // [3 row tiles][KB][hi,lo][64 lanes] A-operand fragments: row 4 t + h = tap t, hidden unit h
    const float *bias0, *w1;    // [4] folded first-layer biases, second-layer weights (zero padded)
    const double *thresholds;   // [1]
};
// ---- frames of whole hops (W = N = R hop, R = 4, 2 or 1): every block of `hop` samples transformed once on the matrix cores, frames as sliding
// sums of R blocks, the window as three taps along the bins, then the matrix-core network stage -- one launch (kernels_bdft.hip)
constexpr int kBdftBlock = 512;          // 8 waves, two per SIMD; wave w owns bins kb0 + 16 w .. + 15
struct BdftDesc {
    int hop, kb0, f0;           // hop = N / R (128 or 256); first of the 128 bins transformed (a multiple of 4, <= f0 - 1); the band's first bin
    int R;                      // blocks per frame: 4, 2 or 1 (75 %, 50 %, no overlap)
    float a0, a1c, a1s;         // the window as a cosine sum: a_0, (a_1 / 2) cos(pi hop / N), (a_1 / 2) sin(pi hop / N)
    const uint4 *basis;         // [8 waves][cosine rows, sine rows][hop / 64 k-steps][hi,lo][64 lanes] A-operand fragments of the folded block basis
    const float *cre;           // [8 waves][64 lanes][4] the block's first sample's real coefficients for the lane's bins
    const uint4 *afrag;         // [3 row tiles][4][hi,lo][64 lanes] first layer, all taps as rows, K = bin - kb0
};
// outputs [C][E][1], flags [C][E] <- samples [C][stride]; S: samples per channel
hipError_t launch_bdft_net(const MlpxDesc &d, const BdftDesc &bd, const float *samples, int64_t stride, int C, int64_t S, int64_t J, int64_t E,
                           float *outputs, uint8_t *flags, hipStream_t stream);
// ---- 1024-point frames: packed real FFT + the matrix-core network stage in one launch (kernels_fft1k.hip) ----
constexpr int kFft1kBlock = 768;         // 12 waves (three per SIMD): a frame per wave at a time, 10 or 11 frames of a 128-frame tile each
bool fft1k_applicable(const StftDesc &s, const MlpxDesc &d, const float *samples, int64_t stride);
// outputs [C][E][1], flags [C][E] <- samples [C][stride]
hipError_t launch_fft1k_net(const StftDesc &s, const MlpxDesc &d, const float *samples, int64_t stride, int C, int64_t J, int64_t E,
                            float *outputs, uint8_t *flags, hipStream_t stream);
// outputs [C][E][1], flags [C][E] <- columns [C][J][F]
hipError_t launch_mlpx(const MlpxDesc &d, const float *columns, int C, int64_t J, int64_t E, float *outputs, uint8_t *flags,
                       hipStream_t stream);

// ResamplerLinear (Common/Resampler.swift:36-69) for C channels at once; `last` is the per-channel carry on the device
hipError_t launch_resample_linear(const float *in, int64_t n_in, int64_t in_stride, float *out, int64_t n_out,
                                  int64_t out_stride, int C, float step, float offset, float *last, hipStream_t stream);
// whole-recording rate conversion, fp64 positions (offline input: no carry)
hipError_t launch_convert_rate(const float *in, int64_t n_in, int64_t in_stride, float *out, int64_t n_out, int64_t out_stride,
                               int C, double step, hipStream_t stream);
// ---- band-limited whole-recording rate conversion (kernels_sinc.hip; the sinc convention of include/syldet.h) ----
constexpr int kSincPerThread = 4;                     // outputs a thread, 256 apart
constexpr int kSincBlockOut = 256 * kSincPerThread;   // consecutive outputs of one row a workgroup
constexpr int kSincStage = 4000;                      // input samples staged in LDS at a time
// entries N of the unit filter's table over [0, Z]: at least 512 a zero crossing, a multiple of 4; the table holds N + 4 floats,
// g[j] = sinc(j Z / N) * kaiser(j / N) for j < N and zeros from g[N] on
inline int sinc_table_entries(int Z) { return Z <= 32 ? 16384 : 32768; }
// in [C][in_stride] -> out [C][out_stride]; H = Z / s (|H| <= 65536), scale = float(s), table on the device, 16-byte aligned
hipError_t launch_convert_rate_sinc(const float *in, int64_t n_in, int64_t in_stride, float *out, int64_t n_out,
                                    int64_t out_stride, int C, double rate_in, double rate_out, double H, float scale,
                                    const float *table, int N, hipStream_t stream);
// the streaming form: the outputs m0 .. m0 + n_emit - 1 of a stream of n_before samples so far into out[C][out_stride], read from
// hist [C][L] (the last min(n_before, L) samples, fp32) and the pushed rows in [C][in_stride] of n_in samples (a flush: n_in = 0,
// in unused); then, when n_in > 0, the next history into next [C][L] (another buffer).  At most two kernels.  sinc_stream.hpp
hipError_t launch_sinc_stream_push(const float *hist, float *next, int64_t L, const float *in, int64_t n_in, int64_t in_stride,
                                   int64_t n_before, float *out, int64_t out_stride, int64_t m0, int64_t n_emit, int C,
                                   double rate_in, double rate_out, double H, float scale, const float *table, int N,
                                   hipStream_t stream);
hipError_t launch_sinc_stream_push_s16(const float *hist, float *next, int64_t L, const int16_t *in, int64_t n_in, int64_t in_stride,
                                       int64_t n_before, float *out, int64_t out_stride, int64_t m0, int64_t n_emit, int C,
                                       double rate_in, double rate_out, double H, float scale, const float *table, int N,
                                       hipStream_t stream);
hipError_t launch_convert_rate_sinc_s16(const int16_t *in, int64_t n_in, int64_t in_stride, float *out, int64_t n_out,
                                        int64_t out_stride, int C, double rate_in, double rate_out, double H, float scale,
                                        const float *table, int N, hipStream_t stream);
// frame-major [n_frames][total] -> channel-major rows of channels first .. first+C-1
hipError_t launch_deinterleave(const float *in, int64_t n_frames, int total, int first, int C, float *out,
                               int64_t out_stride, hipStream_t stream);
// the same for 16-bit PCM: frame-major int16 [n_frames][total] -> int16 rows of channels 0 .. C-1
hipError_t launch_deinterleave_s16(const int16_t *in, int64_t n_frames, int total, int C, int16_t *out, int64_t out_stride,
                                   hipStream_t stream);
// 16-bit PCM rows [C][in_stride] -> fp32 rows [C][out_stride] of x * 2^-15 (exact); out 16-byte aligned, out_stride % 4 == 0
hipError_t launch_widen_s16(const int16_t *in, int64_t in_stride, int64_t S, int C, float *out, int64_t out_stride, hipStream_t stream);

// ---- the Simulator's output track (kernels_trace.hip; ViewControllerSimulator.swift:251-344) ----
// outputs [C][n_evals][n_out], thr [C] = Float(thresholds[k]) of each channel's network -> trace [C][stride] (the first n_samples of
// each row): 0 in front of first_index, clamp01(out[e][k] / thr[c]) over the hop samples of evaluation e, 0 behind the last one.
// fp32: the reference's values; int16: rint(v * 32767), NaN -> 0.
hipError_t launch_trace(const float *outputs, int64_t n_evals, int n_out, int k, const float *thr, int C, float *trace,
                        int64_t n_samples, int64_t stride, int64_t first_index, int64_t hop, hipStream_t stream);
hipError_t launch_trace_s16(const float *outputs, int64_t n_evals, int n_out, int k, const float *thr, int C, int16_t *trace,
                            int64_t n_samples, int64_t stride, int64_t first_index, int64_t hop, hipStream_t stream);
// the int16 form frame-major, frames [n_frames][C] (one channel: the planar kernel)
hipError_t launch_trace_interleaved_s16(const float *outputs, int64_t n_evals, int n_out, int k, const float *thr, int C,
                                        int16_t *frames, int64_t n_frames, int64_t first_index, int64_t hop, hipStream_t stream);

// ---- the TTL trigger track (kernels_trigger.hip; Processor.swift:128-148, AudioInterface.swift:13-40, :442-445) ----
// B' of include/syldet.h: entries of one channel's last_seen row for a recording of n_samples (-1: too long for 32-bit buffers)
int64_t trigger_buffers(int64_t n_samples, int L);
// flags [C][n_evals] -> last_seen [C][B'] int32: the greatest seen buffer <= b, or -1 (trigger_scan_kernel)
hipError_t launch_trigger_scan(const uint8_t *flags, int64_t n_evals, int C, int L, int64_t n_samples, int64_t first_index, int64_t hop,
                               int *last_seen, hipStream_t stream);
// last_seen -> track [C][stride] (the first n_samples of each row): fp32 1.0f / 0.0f, int16 32767 / 0 (trigger_kernel)
hipError_t launch_trigger(const int *last_seen, int C, int L, int64_t N, int64_t Lat, float *track, int64_t n_samples, int64_t stride,
                          hipStream_t stream);
hipError_t launch_trigger_s16(const int *last_seen, int C, int L, int64_t N, int64_t Lat, int16_t *track, int64_t n_samples, int64_t stride,
                              hipStream_t stream);
// the int16 form frame-major: samples == nullptr, frames [n_frames][C] (one channel: the planar kernel); else frames [n_frames][2 C],
// channel c's audio (samples [C][sample_stride] int16, copied bit for bit) at lane 2 c and its trigger at 2 c + 1
hipError_t launch_trigger_interleaved_s16(const int *last_seen, int C, int L, int64_t N, int64_t Lat, const int16_t *samples,
                                          int64_t sample_stride, int16_t *frames, int64_t n_frames, hipStream_t stream);
// the rising edges' sample numbers in order, indices [C][capacity] and counts [C] as launch_detections writes them
hipError_t launch_trigger_onsets(const int *last_seen, int C, int L, int64_t N, int64_t Lat, int64_t n_samples, int64_t *indices,
                                 int64_t capacity, int64_t *counts, hipStream_t stream);

// ---- the level meters (kernels_levels.hip; Processor.swift:111-113, :138, :158-184) ----
// what a workgroup of levels_in_kernel leaves of a reading that reaches into a neighbour: the greatest mean square of its buffers
// that is not NaN (-1: none), and the reading's first value where the workgroup holds its first buffer
struct LevelsPartial {
    double best, first;
};
// scratch launch_levels_in needs for rows of n_samples (two partials a workgroup)
size_t levels_scratch_bytes(int64_t n_samples, int C, int L, bool s16);
// samples [C][stride] fp32 or (s16) int16 -> mean_square [C][M] fp64, M = ceil(ceil(n_samples / L) / P): the StatMax over the P
// buffers of a reading of Double(sum_squares_tree(buffer)) / Double(length).  *needs_fold: readings cross workgroups, and
// launch_levels_fold (levels_fold_kernel) has to follow on the same stream with the same arguments.
hipError_t launch_levels_in(const void *samples, bool s16, int C, int64_t n_samples, int64_t stride, int L, int64_t P, double *mean_square,
                            void *scratch, hipStream_t stream, bool *needs_fold);
hipError_t launch_levels_fold(const void *scratch, bool s16, int C, int64_t n_samples, int L, int64_t P, double *mean_square, hipStream_t stream);
// outputs [C][n_evals][n_out] -> levels [C][M] fp32: the StatMax of output k over the evaluations of each reading (need = gap +
// window, T = timeRange: syldet_count_evals' rule), 0 for a reading without one
hipError_t launch_levels_out(const float *outputs, int64_t n_evals, int n_out, int k, int C, int64_t n_samples, int L, int64_t P,
                             int64_t need, int64_t hop, int T, float *levels, hipStream_t stream);

// ---- packed recordings (kernels_recordings.hip; syldet_recordings_* of include/syldet.h) ----
// One slot of the plan as the load kernel reads it: the table is sorted by (row, offset), row c's slots are
// [row_begin[c], row_begin[c + 1]).  Sample i of the slot is src[src_offset + i src_step] -- or, for a source of the files' own bytes
// (format: one of pcm_values.hpp's, else 0), the `format` value at byte src_offset + i src_step.
struct RecSlotDev {
    int64_t offset, n_samples, src_offset;
    int32_t src_step, format;
};
// ... and as the events kernel reads it, in the caller's order of recordings
struct RecEventDev {
    int64_t first_eval, n_evals;
    int32_t row, pad;
};
constexpr int kRecTile = 8192;               // samples of a row one workgroup of recordings_load_kernel writes
struct RecLoadDesc {
    const RecSlotDev *slots;
    const int32_t *row_begin;                // [C + 1]
    const int32_t *tile_first;               // [C][tiles]: the last slot of the row that starts at or before the tile (row_begin[c + 1]: none)
    int tiles;                               // ceil(row_samples / kRecTile)
    int64_t row_samples;                     // a multiple of 8
};
// rows [C][stride] (the first row_samples of each) <- the recordings' samples and +0 everywhere else; fp32 or (s16) int16
hipError_t launch_recordings_load(const RecLoadDesc &d, const void *src, bool s16, void *rows, int64_t stride, int C, hipStream_t stream);
// the same rows, fp32, from the files' own bytes: every slot decoded from its format (kernels_recordings_pcm.hip)
hipError_t launch_recordings_load_pcm(const RecLoadDesc &d, const void *src, float *rows, int64_t stride, int C, hipStream_t stream);
// indices [K][capacity], values [K][capacity][n_out] (or null), counts [K] <- flags [C][row_evals], outputs [C][row_evals][n_out] (or null)
hipError_t launch_recordings_events(const RecEventDev *desc, int K, int64_t row_evals, int n_out, const float *outputs, const uint8_t *flags,
                                    int64_t first_index, int64_t hop, int64_t debounce_frames, int64_t *indices, float *values,
                                    int64_t capacity, int64_t *counts, hipStream_t stream);

// ---- packed recordings at other rates (kernels_recordings_sinc.hip; syldet_recordings_load_sinc_device* of include/syldet.h) ----
// One slot of the plan as the converting load reads it, in the order of RecSlotDev's table.  Its span is [offset, span_end): up to
// the next recording's offset in the row, or to row_samples behind the row's last.  Positions [offset, offset + n_out) are the
// recording's outputs (copy: its own samples, n_out <= n_in), the rest of the span is +0.
struct RecSincDev {
    int64_t offset, n_out, span_end, src_offset, n_in;
    double rate_in, H;                       // the recording's rate; H = Z / s of its design
    float scale, idx_scale;                  // float(s); float(N / H)
    int32_t src_step;
    int16_t copy, format;                    // copy: at the network's rate, not converted; format: RecSlotDev's (a byte source), else 0
};
struct RecSincDesc {
    const RecSincDev *slots;
    const int32_t *row_begin;                // [C + 1] (RecLoadDesc's)
    // row c's slots own consecutive workgroups of the row: slot row_begin[c] + j the workgroups [wg[j], wg[j + 1]) with wg =
    // wg_begin + row_begin[c] + c, n_c + 1 entries a row (wg[0] = 0, wg[n_c] the row's count): K + C words in all, which the
    // kernel searches with its block index
    const int32_t *wg_begin;
    int grid_x;                              // the greatest count of a row; ceil(row_samples / kSincBlockOut) where a row has no recording
    int64_t row_samples;
};
// rows [C][stride] fp32 (the first row_samples of each) <- every recording converted to rate_out (or copied), +0 everywhere else;
// src fp32 or (s16) int16; table: the unit filter's N + 4 floats on the device, 16-byte aligned
hipError_t launch_recordings_load_sinc(const RecSincDesc &d, const void *src, bool s16, double rate_out, const float *table, int N,
                                       float *rows, int64_t stride, int C, hipStream_t stream);
// ... and src the files' own bytes, every slot in its format
hipError_t launch_recordings_load_sinc_pcm(const RecSincDesc &d, const void *src, double rate_out, const float *table, int N, float *rows,
                                           int64_t stride, int C, hipStream_t stream);

// ---- packed recordings: the per-sample tracks (kernels_recordings_tracks.hip; syldet_recordings_trace_device* and
// syldet_recordings_trigger*_device* of include/syldet.h) ----
// Where one slot's track goes, in the order of RecSlotDev's table: element i at dst[dst_offset + i dst_step].  k: the recording, its
// index in the caller's order (RecEventDev's, ls_begin's, n_samples').
struct RecTrackDev {
    int64_t dst_offset;
    int32_t dst_step, k;
};
struct RecTrackDesc {
    RecLoadDesc load;                        // the plan's slots, rows and tiles: the load's own tables
    const RecEventDev *events;               // [K]
    const RecTrackDev *dst;                  // [K] the kept destination layout
    const int32_t *ls_begin;                 // [K + 1] recording k's last_seen table is entries [ls_begin[k], ls_begin[k + 1]) (the kept L)
    const int64_t *n_samples;                // [K]
    int K;
    int64_t row_evals;
};
// outputs [C][row_evals][n_out], thr [C] -> every recording's trace at its destination; dst fp32 or (s16) int16
hipError_t launch_recordings_trace(const RecTrackDesc &d, int C, const float *outputs, int n_out, int k, const float *thr, void *dst, bool s16,
                                   int64_t first_index, int64_t hop, hipStream_t stream);
// flags [C][row_evals] -> last_seen: every recording's table (trigger_buffers(n_k, L) entries), end to end
hipError_t launch_recordings_trigger_scan(const RecTrackDesc &d, const uint8_t *flags, int L, int64_t first_index, int64_t hop, int *last_seen,
                                          hipStream_t stream);
// last_seen -> every recording's trigger track at its destination
hipError_t launch_recordings_trigger(const RecTrackDesc &d, int C, const int *last_seen, int L, int64_t N, int64_t Lat, void *dst, bool s16,
                                     hipStream_t stream);
// last_seen -> indices [K][capacity], counts [K]
hipError_t launch_recordings_trigger_onsets(const RecTrackDesc &d, const int *last_seen, int L, int64_t N, int64_t Lat, int64_t *indices,
                                            int64_t capacity, int64_t *counts, hipStream_t stream);

// ---- packed recordings: the level meters (kernels_recordings_levels.hip; syldet_recordings_levels_device* and
// syldet_recordings_output_levels_device of include/syldet.h) ----
struct RecLevelsDesc {
    RecLoadDesc load;                        // the plan's slots, rows and tiles: the load's own tables
    const RecEventDev *events;               // [K]
    const int64_t *n_samples;                // [K]
    const int64_t *reading_first;            // [K + 1] recording k's readings are [reading_first[k], reading_first[k + 1]) (the kept L, P)
    const int64_t *slot_first;               // [K] the same starts in the order of RecSlotDev's table
    int K;
    int64_t row_evals, n_readings;           // n_readings = reading_first[K]
};
// mean_square [n_readings] <- +0: in front of launch_recordings_levels_in wherever a row has two tiles (a reading may cross them)
hipError_t launch_recordings_levels_zero(double *mean_square, int64_t n_readings, hipStream_t stream);
// rows [C][stride] fp32 or (s16) int16 -> mean_square [n_readings] fp64: every recording's launch_levels_in, alone
hipError_t launch_recordings_levels_in(const RecLevelsDesc &d, int C, const void *rows, bool s16, int64_t stride, int L, int64_t P,
                                       double *mean_square, hipStream_t stream);
// outputs [C][row_evals][n_out] -> levels [n_readings] fp32: every recording's launch_levels_out, alone
hipError_t launch_recordings_levels_out(const RecLevelsDesc &d, int C, const float *outputs, int n_out, int k, int L, int64_t P, int64_t need,
                                        int64_t hop, int T, float *levels, hipStream_t stream);

// ---- threshold calibration (kernels_score.hip; syldet_score_device of include/syldet.h) ----
// What a scorer keeps on the device.  A detector is a channel (slots == nullptr: its evaluations are row `det`) or a recording
// (slots [D], detector_spans.hpp in evaluations: its own part of its row).
struct ScoreDesc {
    const float *thresholds;                 // [K] the smallest float >= each threshold (score_scan.hpp)
    const float *group_least;                // [ceil(K / 64)] the least of each group of 64
    const int64_t *labels;                   // every detector's sorted labels, end to end
    const int64_t *label_begin;              // [D + 1] detector d's labels are [label_begin[d], label_begin[d + 1])
    const DetSpan *slots;
    int K;
    int64_t tolerance, debounce_frames;
};
// table [D][K][6] int64 <- output `output` of outputs [rows][n_evals][n_out]; one launch (score_kernel)
hipError_t launch_score(const ScoreDesc &d, int D, const float *outputs, int64_t n_evals, int n_out, int output, int64_t first_index,
                        int64_t hop, int64_t *table, hipStream_t stream);

// ---- event-aligned windows (kernels_align.hip; syldet_align_device and syldet_align_stats_device of include/syldet.h) ----
// What an aligner keeps on the device for the windows.  dets == nullptr: detector d is row d, from unit 0, with the call's n_units.
struct AlignDesc {
    const DetSpan *dets;                     // [D] a packed plan's detectors in the source's unit (detector_spans.hpp)
    const int64_t *event_begin;              // [D + 1] the kept prefix
    int2 *spans;                             // [N] each window's present elements (first, count): what the statistics count by
    int D, width;
    int64_t origin, step, before, after;     // the source's anchor rule and the window (align_span.hpp)
};
// windows [N][n * width] <- src [rows][row_stride], events as include/syldet.h states them; one launch (align_windows_kernel)
hipError_t launch_align_windows(const AlignDesc &d, const float *src, int64_t n_units, int64_t row_stride, const int64_t *events,
                                int64_t event_stride, int64_t N, float fill, float *windows, hipStream_t stream);
// ... and for the stack statistics: the events in group order, in blocks of 256.
constexpr int kAlignBlock = 256;             // events a block of the statistics' tree
struct AlignStatsDesc {
    const int64_t *perm;                     // [N] the window of the group-ordered event i
    const int64_t *group_begin;              // [G + 1] group g's events are i in [group_begin[g], group_begin[g + 1])
    const int64_t *block_begin;              // [G + 1] ... and its blocks [block_begin[g], block_begin[g + 1])
    const int32_t *block_group;              // [B]
    const int2 *spans;                       // [N]
    int64_t *part_count;                     // [B][L] the blocks' partials: scratch
    double *part_sum, *part_sumsq;
    int G;
    int64_t B;
};
// part_* [B][L] <- windows [N][L] (align_stats_kernel), then count, sum, sumsq [G][L] <- part_* in block order (align_combine_kernel)
hipError_t launch_align_stats(const AlignStatsDesc &d, const float *windows, int L, hipStream_t stream);
hipError_t launch_align_combine(const AlignStatsDesc &d, int L, int64_t *count, double *sum, double *sumsq, hipStream_t stream);

// ---- training (kernels_train.hip; syldet_train_targets_device and syldet_train_gradient_device of include/syldet.h) ----
struct TrainTargetsDesc {
    const DetSpan *dets;                     // packed plans: the by_row table in evaluations (detector_spans.hpp); nullptr: detector c is row c, all of it
    const int32_t *row_begin;                // [rows + 1]
    const int64_t *labels;                   // every detector's sorted labels, end to end
    const int64_t *label_begin;              // [D + 1]
    const int32_t *label_output;             // [n_labels], or nullptr: all 0
    int rows, n_out;
    int64_t first_index, hop, half_width;
    float weight_positive, weight_negative;
};
// targets [rows][n_evals][n_out], weights [rows][n_evals]: every element written (train_targets.hpp)
hipError_t launch_train_targets(const TrainTargetsDesc &d, int64_t n_evals, float *targets, float *weights, hipStream_t stream);
// The network as the gradient kernel reads it: everything but the two layers' parameters, which come with every call.
struct TrainDesc {
    int F, T, I, H, O;                       // bins, timeRange, F T, hidden units, outputs
    int tf0, tf1, scaling;
    int n_in_fns, n_out_fns;
    DevFn in_fns[kMaxFns], out_fns[kMaxFns]; // xoff / gain: offsets into maps
    const float *maps;                       // the map functions' x offsets and gains
    // the launch shape, a function of the numbers above alone (train_plan)
    int HP;                                  // H padded to 4, 8 or 16
    int threads, tile, FP;                   // threads a workgroup; evaluations a tile (<= threads); floats a staged frame (odd)
    int lds_stage, lds_d1, lds_stats, lds_red, lds_sel, lds_total;   // byte offsets behind the transposed first layer
    int max_groups;                          // the most workgroups a launch takes (each keeps P + 2 doubles of partial sums)
};
inline int train_param_count(int I, int H, int O) { return H * I + H + O * H + O; }
bool train_plan(TrainDesc &d);               // false: the shape does not fit the kernel
hipError_t train_prepare(const TrainDesc &d);    // on the trainer's device, once: the kernel's LDS above 64 KB allowed
int train_groups(const TrainDesc &d, int rows, int64_t n_evals);   // workgroups of a launch: min(tiles, max_groups)
// part [groups][P + 2] fp64 <- the groups' partial gradients, loss and weight sum (train_gradient_kernel); then loss [2], gradient [P]
// <- the partials added in group order, rounded once (train_combine_kernel)
hipError_t launch_train_gradient(const TrainDesc &d, const float *columns, int64_t row_stride, int rows, const float *params, const float *targets,
                                 const float *weights, int64_t n_evals, double *part, hipStream_t stream);
hipError_t launch_train_combine(const TrainDesc &d, int groups, const double *part, double *loss, float *gradient, hipStream_t stream);
// the input range in front of input function `at` (train_first_map: the first mapminmax, -1 without one): part as above <- the
// groups' least and greatest [2][I] floats and their int64 counts (train_range_kernel); then range [2][I], count [1]
// (train_range_combine_kernel; groups 0: {+inf, -inf} and 0)
int train_first_map(const TrainDesc &d);
hipError_t launch_train_range(const TrainDesc &d, int at, const float *columns, int64_t row_stride, int rows, const float *weights, int64_t n_evals,
                              double *part, hipStream_t stream);
hipError_t launch_train_range_combine(const TrainDesc &d, int groups, const double *part, float *range, int64_t *count, hipStream_t stream);
// one Adam step on params [P] in place (train_adam.hpp; kernels_train_adam.hip): loss {L, Wsum} and gradient as the combine kernel
// left them, read on the device; mean_loss (may be NULL) <- L / Wsum
struct TrainAdamStep;
hipError_t launch_train_adam(const TrainAdamStep &k, int P, const double *loss, const float *gradient, float *m, float *v, float *params, double *mean_loss,
                             hipStream_t stream);
// The multi form (syldet_trainer_create_multi): a network per row.  The tables lie on the device from creation: every network's
// own TrainDesc (its maps and its functions' y; the shape and the launch shape are shared), the bank's rows sorted by network
// (ascending within one) and where each network's rows begin.  The grid is (min(max_rows x tiles a row, max_groups), N):
// workgroup g of network n leaves at once unless g < G_n = min(network n's tiles, max_groups), and else is workgroup g of G_n of a
// plain launch over that network's rows alone -- the same tiles in the same order, partial n max_groups + g.  params [N][P];
// loss [N][2], gradient [N][P]; range [N][2][I], count [N]; the Adam step's moments and mean_loss [N].
struct TrainMulti {
    const TrainDesc *descs;                  // [N]
    const int32_t *rows;                     // [rows] sorted by network
    const int32_t *net_row_begin;            // [N + 1]
    int n_nets, max_rows;                    // max_rows: the most rows one network has
};
hipError_t train_prepare_multi(const TrainDesc &d);
hipError_t launch_train_gradient_multi(const TrainDesc &d, const TrainMulti &mu, const float *columns, int64_t row_stride, const float *params,
                                       const float *targets, const float *weights, int64_t n_evals, double *part, hipStream_t stream);
hipError_t launch_train_combine_multi(const TrainDesc &d, const TrainMulti &mu, int64_t n_evals, const double *part, double *loss, float *gradient,
                                      hipStream_t stream);
hipError_t launch_train_range_multi(const TrainDesc &d, const TrainMulti &mu, int at, const float *columns, int64_t row_stride, const float *weights,
                                    int64_t n_evals, double *part, hipStream_t stream);
hipError_t launch_train_range_combine_multi(const TrainDesc &d, const TrainMulti &mu, int64_t n_evals, const double *part, float *range, int64_t *count,
                                            hipStream_t stream);
hipError_t launch_train_adam_multi(const TrainAdamStep &k, int P, int n_nets, const double *loss, const float *gradient, float *m, float *v, float *params,
                                   double *mean_loss, hipStream_t stream);

// ---- template matching (kernels_match.hip; syldet_match_scores_device and syldet_match_peaks_device of include/syldet.h) ----
constexpr int kMatchTile = 256;              // positions a workgroup of the score kernels takes
constexpr int kMatchChunk = 2048;            // positions a step of the peaks kernel takes
struct MatchDesc {
    const DetSpan *by_row;                   // packed plans: the by_row table in frames (detector_spans.hpp), row c's detectors are [row_begin[c], row_begin[c + 1]);
    const int32_t *row_begin;                //   nullptr: detector c is row c, all of it
    const DetSpan *by_det;                   // packed plans: [D] in the caller's order
    const float *templ;                      // t^ [n][bins]
    int rows, D, n, bins, anchor;
    int64_t origin, hop;
    // the score kernel's form, a function of n and bins alone (match_plan)
    int matrix;                              // 1: the Toeplitz form on the matrix cores; 0: one thread a position, plain multiply-adds
    int Fp, FT;                              // floats a staged frame (bins padded to 4); floats a staged template frame (4 x an odd number)
    int lds_bytes;
};
void match_plan(MatchDesc &d);
hipError_t match_prepare();                  // on the matcher's device, once: the peaks kernel's LDS above 64 KB allowed
// scores [rows][n_frames] <- columns [rows][row_stride]: every element written once; one launch (match_scores_mfma_kernel or
// match_scores_plain_kernel)
hipError_t launch_match_scores(const MatchDesc &d, const float *columns, int64_t n_frames, int64_t row_stride, float *scores, hipStream_t stream);
// events [D][capacity], counts [D], event_scores [D][capacity] or nullptr <- scores [rows][n_frames]; one launch (match_peaks_kernel)
hipError_t launch_match_peaks(const MatchDesc &d, const float *scores, int64_t n_frames, float threshold, int separation, int64_t *events,
                              int64_t capacity, int64_t *counts, float *event_scores, hipStream_t stream);
// A bank of K templates in C classes ("template matching: a bank of templates" of include/syldet.h): d.templ is [K][n][bins], the
// form and the LDS of a tile are match_plan's, which K does not enter.
struct MatchBankDesc {
    MatchDesc d;
    const int32_t *order;                    // [K] the templates class by class, ascending k within a class (on the device)
    const int32_t *order_class;              // [K] the class of order[i]
    int K, C;
};
struct MatchBankKeys {
    uint32_t key[16];                        // match_key of every class's threshold
};
hipError_t match_bank_prepare();             // as match_prepare, for the bank's peaks kernel
// scores [C][rows][n_frames], which [C][rows][n_frames] or nullptr <- columns; every element written once; one launch
// (match_bank_scores_mfma_kernel or match_bank_scores_plain_kernel)
hipError_t launch_match_bank_scores(const MatchBankDesc &b, const float *columns, int64_t n_frames, int64_t row_stride, float *scores, int32_t *which,
                                    hipStream_t stream);
// events [C][D][capacity], counts [C][D], event_scores and event_template [C][D][capacity] or nullptr <- scores and which
// [C][rows][n_frames]; one launch (match_bank_peaks_kernel), grid (D, C)
hipError_t launch_match_bank_peaks(const MatchBankDesc &b, const float *scores, const int32_t *which, int64_t n_frames, const float *thresholds,
                                   int separation, int64_t *events, int64_t capacity, int64_t *counts, float *event_scores, int32_t *event_template,
                                   hipStream_t stream);
// ... with a separation a class, passed by value beside the keys (match_bank_peaks_each_kernel); LDS by the greatest of them
struct MatchBankSeps {
    int32_t S[16];
};
hipError_t launch_match_bank_peaks_each(const MatchBankDesc &b, const float *scores, const int32_t *which, int64_t n_frames, const float *thresholds,
                                        const int32_t *separations, int64_t *events, int64_t capacity, int64_t *counts, float *event_scores,
                                        int32_t *event_template, hipStream_t stream);
// A ragged bank ("template matching: a ragged bank" of include/syldet.h; match_ragged.hpp): template k is [len[k]][bins] at
// d.templ + offset[k], its window at plane element u the frames [u - anchor[k], u - anchor[k] + len[k]).  d.n: the greatest
// length; d.Fp, d.FT, d.matrix, d.lds_bytes: match_ragged_plan's.  The planes are indexed by the anchor frame.
struct MatchRaggedDesc {
    MatchDesc d;
    const int32_t *order, *order_class;      // [K] as MatchBankDesc's
    const int32_t *len, *anchor, *offset;    // [K] by template (on the device)
    int K, C;
    int a_max, G;                            // the staged frames of a tile begin a_max in front of its first element; their number
};
// scores and which [C][rows][n_frames] <- columns; every element written once; one launch (match_ragged_scores_mfma_kernel or
// match_ragged_scores_plain_kernel)
hipError_t launch_match_ragged_scores(const MatchRaggedDesc &b, const float *columns, int64_t n_frames, int64_t row_stride, float *scores,
                                      int32_t *which, hipStream_t stream);

// detection flags <-> bits (bit b of byte t of a row = flag 8 t + b), rows padded to whole bytes
hipError_t launch_pack_flags(const uint8_t *flags, int64_t rows, int64_t row_len, uint8_t *bits, hipStream_t stream);
hipError_t launch_unpack_flags(const uint8_t *bits, int64_t rows, int64_t row_len, uint8_t *flags, hipStream_t stream);
hipError_t launch_unpack_flags_gathered(const uint8_t *bits, int64_t rows, int64_t row_len, int64_t shards, int64_t padded,
                                        uint8_t *flags, hipStream_t stream);
// (the copy exchange: every shard's packed rows behind a pointer of its own, read where they lie)
constexpr int kMaxFlagSources = 16;
struct FlagSources {
    const uint8_t *p[kMaxFlagSources] = {};
};
hipError_t launch_unpack_flags_from(const FlagSources &from, int64_t rows, int64_t row_len, int64_t shards, int64_t padded,
                                    uint8_t *flags, hipStream_t stream);

// ---- which instantiation ran (the tests' seam: syldet_last_fused_form, syldet_fused_form_of_config) ----
// Every launch_one of the three fused kernel files leaves its template arguments here before its first HIP call: kernel as in
// fused_choice (0 the 8-wave kernel, 1 the register-resident-basis kernel, 2 the symmetric-fold kernel), p the arguments in
// declaration order, defaulted ones included (booleans as 0 / 1), zero behind the last.  Under `dry` it then returns hipSuccess
// without touching the device: the launchers themselves say which form a plan takes, nothing restates their routing.
struct FusedForm {
    int kernel;
    int p[10];
};
struct FusedSeam {
    FusedForm last;
    bool dry;
};
FusedSeam &fused_seam();        // the calling thread's (fused_plan.cpp)
inline bool fused_note_form(int kernel, int p0, int p1, int p2, int p3, int p4, int p5, int p6 = 0, int p7 = 0, int p8 = 0, int p9 = 0)
{
    FusedSeam &s = fused_seam();
    s.last = FusedForm{kernel, {p0, p1, p2, p3, p4, p5, p6, p7, p8, p9}};
    return s.dry;
}

// mn: a multi-network handle's tables (only the fold kernel has that form: anything else is hipErrorInvalidValue)
// s16: `samples` are int16 rows (16-bit PCM, x * 2^-15), only where fused_s_native_s16(d) and the fold kernel is chosen
hipError_t launch_fused(const FusedDesc &d, const float *samples, int64_t stride, int C, int64_t S, int64_t J,
                        int64_t E, float *outputs, uint8_t *flags, hipStream_t stream, const FusedMulti *mn = nullptr, bool s16 = false);
int fused_choice(const FusedDesc &d, int64_t J);    // 0 the 8-wave kernel, 1 the register-resident-basis kernel, 2 the symmetric-fold kernel
// the DFT front half alone: samples -> [C][J][F] columns; d: a plan for timeRange 1 with spect_out / spect_power set
hipError_t launch_fused_spectrogram(const FusedDesc &d, const float *samples, int64_t stride, int C, int64_t J, hipStream_t stream);
// ... on the symmetric-fold kernel's twice-folded form, where the plan allows it (256-point frames under a 256-sample window)
bool fused_s_spectrogram_applicable(const FusedDesc &d);
hipError_t launch_fused_s_spectrogram(const FusedDesc &d, const float *samples, int64_t stride, int C, int64_t J, hipStream_t stream);
// the same contract on the register-resident-basis kernel; only called when d.r_ok and fused_r_applicable(d)
bool fused_r_applicable(const FusedDesc &d);
bool fused_r_has_stamps();      // built with -DSYLDET_R_STAMPS (phase timing, SYLDET_FUSED_STAMPS=1)
bool fused_s_has_stamps();      // built with -DSYLDET_S_STAMPS: where a wave of the fold kernel waits (SYLDET_FUSED_STAMPS=1)
hipError_t launch_fused_r(const FusedDesc &d, const float *samples, int64_t stride, int C, int64_t S, int64_t J,
                          int64_t E, float *outputs, uint8_t *flags, hipStream_t stream);
// the same contract on the symmetric-fold kernel; only called when fused_s_applicable(d)
bool fused_s_applicable(const FusedDesc &d);
hipError_t launch_fused_s(const FusedDesc &d, const float *samples, int64_t stride, int C, int64_t S, int64_t J,
                          int64_t E, float *outputs, uint8_t *flags, hipStream_t stream, const FusedMulti *mn = nullptr, bool s16 = false);
// Does the launcher run this plan on a form with a 16-bit PCM twin (the twice-folded form on the plain ring, one quad of units,
// eight waves)?  The caller also needs rows of whole 4-byte words: int16 rows 4-byte aligned, an even stride, an even gap.
bool fused_s_native_s16(const FusedDesc &d);
// taps the register-resident first-layer fragments are instantiated for (0: timeRange too long)
int fused_taps_max(int T);

// ---- exact recomputation of the evaluations the fused kernels reported (kernels_fixup.hip) ----
struct FixDesc {
    int N, W, hop, gap, f0, F, T;
    int power_mode;             // spectrogram items: 0 |X| (extractPower), 1 |X|^2 (extractMagnitude)
    const float *window;        // [W] the fp32 window table (WindowType.createWindow)
    const double2 *ctab;        // [N] (cos, sin)(2 pi m / N)
    int s16;                    // the samples are int16 rows (16-bit PCM: x * 2^-15, exact in fp64 as in fp32)
};
constexpr int kFixMaxCount = 16;            // evaluations (or frames) per work item
// outputs [C][E][n_out], flags [C][E]: the listed evaluations are overwritten; columns [C][J][F]: the listed frames
hipError_t launch_fixup(const FixDesc &fd, const NetDesc &n, const float *samples, int64_t stride, int64_t J, int64_t E,
                        float *outputs, uint8_t *flags, float *columns, const FixList &list, hipStream_t stream);

}  // namespace sd
