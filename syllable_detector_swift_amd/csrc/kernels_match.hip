// kernels_match.hip -- template matching (syldet_match_scores_device, syldet_match_peaks_device of include/syldet.h): the cosine
// between a normalised template t^ [n][bins] and the window of n frames at every position of every detector, and the matches
// among the scores.
//
//   match_scores_mfma_kernel    A workgroup of four waves takes 256 consecutive frames of a row as positions and stages the 255 + n
//                  frames their windows reach in LDS once, bins padded to a multiple of 4 with zeros by selection, frames behind
//                  the row's end likewise.  A thread a frame then takes the frame's energy from the staged values (a chain of
//                  fused multiply-adds over the bins) and replaces a NaN or an Inf by zero, so that a product with a zero of the
//                  Toeplitz operand below cannot carry it into a window that does not hold it; the energy keeps it.  The inner
//                  products run on v_mfma_f32_16x16x4_f32 in the Toeplitz arrangement: row m of the A operand is the frames from
//                  16 m on, column i of the B operand the template shifted down by i frames (zeros by selection above and below
//                  it), so accumulator element (m, i) is position 16 m + i: a chain of fused multiply-adds over the window in
//                  (frame, bin) order in front of and behind which only zeros are added.  (n + 15) / n of the window's products,
//                  no shuffle.  The waves share the k dimension by groups of 4 bins (wave w the groups w, w + 4, ..), every
//                  group's chain is whole, and the waves' sums are added in wave order.  A thread a position adds them, sums
//                  the window's n frame energies from its first frame on, and writes the score or the NaN of a position that
//                  holds none.  LDS: staged frames are 16 m + f at (16 m + f) Fp + 4 m + .., so the 64 lanes of an A read
//                  (m, k) hit 64 banks; the template's frames are 4 x an odd number of floats apart for the same reason.
//   match_scores_plain_kernel   The same sums, one thread a position, from global memory: for shapes whose staged tile does not fit
//                  64 KB of LDS.  Which of the two runs is a function of n and bins alone.
//   match_peaks_kernel          A workgroup a detector walks its positions in steps of 2048: the scores' keys (match_peaks.hpp) of the
//                  step and of S positions on either side go to LDS, log2 S passes of m[i] = max(m[i], m[i + 2^l]) make the maxima of
//                  all windows of 2^k positions, two of which cover any window of S; a thread marks its 8 consecutive positions by
//                  the rule, and a scan over the workgroup's counts places the events in order.
//   match_bank_scores_mfma_kernel, match_bank_scores_plain_kernel, match_bank_peaks_kernel   K templates in C classes in one launch
//                  ("template matching: a bank of templates"): the frames are staged and their energies taken once, every template
//                  then runs the single kernel's products through the same device functions, so template k's score has the single
//                  matcher's bits, and a class's score is the greatest of its templates' (match_classes.hpp); the peaks kernel is
//                  match_peaks_kernel's body a class, grid (D, C).
//   match_ragged_scores_mfma_kernel, match_ragged_scores_plain_kernel, match_bank_peaks_each_kernel   templates of their own lengths
//                  n_k lined up at their anchors a_k ("template matching: a ragged bank"; match_ragged.hpp): a plane is indexed by
//                  the anchor frame, a tile stages max a_k frames in front of its 256 elements and max (n_k - a_k) behind them, and
//                  template k's pass is the bank's with n_k and its first frame a_max - a_k as arguments; a window exists where it
//                  lies inside the detector on both sides.  The third is the bank's peaks kernel with a separation a class.
//
// gfx950 only: wave = 64 lanes.

#include "kernels.hpp"
#include "match_classes.hpp"
#include "match_peaks.hpp"
#include "match_ragged.hpp"

namespace sd {

namespace {

constexpr int kThreads = 256;
constexpr int kOwn = kMatchChunk / kThreads;                 // positions a thread of the peaks kernel marks

static_assert(kMatchTile == kMatchTileElements, "match_ragged.hpp plans the score kernels' tile");

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// A packed plan: the frames [first, end) of the detector of row `row` that starts last at or before frame q; false where the row
// has none.  Whether it still holds q, or a window from q on, is the caller's to ask of `end`.
__device__ __forceinline__ bool match_span(const MatchDesc &d, int row, int64_t q, int64_t &first, int64_t &end)
{
    const int at = span_at_or_before(d.by_row, d.row_begin, row, q);
    if (at < 0) return false;
    const DetSpan e = d.by_row[at];
    first = e.first;
    end = e.first + e.units;
    return true;
}

// Does position q of row `row` hold a score: does a detector's window of n frames begin there?
__device__ __forceinline__ bool match_position(const MatchDesc &d, int row, int64_t q, int64_t n_frames)
{
    if (!d.by_row) return q + d.n <= n_frames;
    int64_t first, end;
    if (!match_span(d, row, q, first, end)) return false;
    return q + d.n <= end;
}

// The frames [first, end) of the detector that holds frame q (a channel: the row); false where none does
__device__ __forceinline__ bool match_holder(const MatchDesc &d, int row, int64_t q, int64_t n_frames, int64_t &first, int64_t &end)
{
    first = 0;
    end = n_frames;
    if (!d.by_row) return true;
    return match_span(d, row, q, first, end) && q < end;
}

// dot: the window's products with t^ (NaN and Inf taken as zero); E: its energy (which keeps them)
__device__ __forceinline__ float match_score(float dot, float E)
{
    if (!finite_bits(E)) return __uint_as_float(0x7fc00000u);
    if (E == 0.0f) return 0.0f;
    return (dot + 0.0f) / sqrtf(E);                          // (-0.0 -> +0.0: zeros added behind a window may have done so already)
}

// ---- the matrix form's phases: one text for match_scores_mfma_kernel and match_bank_scores_mfma_kernel ----
// A tile's LDS: the staged frames, one template, the frames' energies, the waves' sums (match_plan counts the same floats).
struct MatchTile {
    float *X;                                                // frame g, bin b at g Fp + 4 (g >> 4) + b
    float *T;                                                // t^ frame j, bin b at j FT + b
    float *Efr;                                              // [G] the frames' energies
    float *red;                                              // [4][256] the waves' sums
    int G;                                                   // staged frames
};

// G staged frames and a template region of n frames (a ragged bank's: its greatest)
__device__ __forceinline__ MatchTile match_tile_of(float *lds, const MatchDesc &d, int G, int n)
{
    MatchTile t;
    t.G = G;
    t.X = lds;
    t.T = t.X + t.G * d.Fp + 4 * ((t.G + 15) >> 4);
    t.Efr = t.T + n * d.FT;
    t.red = t.Efr + t.G;
    return t;
}

__device__ __forceinline__ MatchTile match_tile(float *lds, const MatchDesc &d) { return match_tile_of(lds, d, kMatchTile - 1 + d.n, d.n); }

// (eight loads a thread in flight: one at a time, the tile's staging waits out a memory latency an element and takes longer
// than its matrix instructions)
constexpr int kStage = 8;

// the frames from p0 on of one row -> X, bins padded to Fp and frames behind the row's end zero by selection (kFront: p0 may lie
// in front of the row's start, and those frames are zero likewise)
template <bool kFront>
__device__ __forceinline__ void match_stage_frames(const MatchDesc &d, const MatchTile &t, const float *__restrict__ src, int64_t p0, int64_t n_frames,
                                                   int tid)
{
    const int bins = d.bins, Fp = d.Fp, G = t.G;
    for (int base = tid; base < G * Fp; base += kThreads * kStage) {
        float v[kStage];
        int at[kStage];
#pragma unroll
        for (int u = 0; u < kStage; u++) {
            const int idx = base + u * kThreads;
            const int g = idx / Fp, b = idx - g * Fp;
            const int64_t gf = p0 + g;
            at[u] = idx < G * Fp ? idx + 4 * (g >> 4) : -1;
            v[u] = 0.0f;
            if (idx < G * Fp && b < bins && gf < n_frames && (!kFront || gf >= 0)) v[u] = src[gf * bins + b];
        }
#pragma unroll
        for (int u = 0; u < kStage; u++)
            if (at[u] >= 0) t.X[at[u]] = v[u];
    }
}

// one template t^ [n][bins] -> T
__device__ __forceinline__ void match_stage_template(const MatchDesc &d, float *T, const float *__restrict__ templ, int n, int tid)
{
    const int bins = d.bins, FT = d.FT;
    for (int base = tid; base < n * FT; base += kThreads * kStage) {
        float v[kStage];
#pragma unroll
        for (int u = 0; u < kStage; u++) {
            const int idx = base + u * kThreads;
            const int j = idx / FT, b = idx - j * FT;
            v[u] = 0.0f;
            if (idx < n * FT && b < bins) v[u] = templ[j * bins + b];
        }
#pragma unroll
        for (int u = 0; u < kStage; u++)
            if (base + u * kThreads < n * FT) T[base + u * kThreads] = v[u];
    }
}

// a thread a frame: its energy from the staged values, and a NaN or an Inf replaced by zero
__device__ __forceinline__ void match_energies(const MatchDesc &d, const MatchTile &t, int tid)
{
    for (int g = tid; g < t.G; g += kThreads) {
        float *x = t.X + g * d.Fp + 4 * (g >> 4);
        float e = 0.0f;
        for (int b = 0; b < d.bins; b++) {
            const float v = x[b];
            e = fmaf(v, v, e);
            if (!finite_bits(v)) x[b] = 0.0f;
        }
        t.Efr[g] = e;
    }
}

// the products of the staged frames with the staged template of n frames: wave w's chains over the bin groups w, w + 4, .. ->
// red[w].  s: the staged frame at which the tile's first window begins (0; a ragged bank: match_ragged_first), so row m of the A
// operand is the frames from 16 m + s on.  The skew 4 (g >> 4) follows the frame g = 16 m + s + f, and (g >> 4) = m + ((s + f) >> 4):
// the lanes of an A read (m, k) are 16 Fp m + 4 m + k floats apart -- 64 banks, Fp being a multiple of 4 -- for any s.
__device__ __forceinline__ void match_products(const MatchDesc &d, const MatchTile &t, int n, int s, int tid)
{
    const int Fp = d.Fp, FT = d.FT;
    const float *X = t.X, *T = t.T;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int groups = Fp >> 2;
    if (wave < groups) {
        const int m = lane & 15, k = lane >> 4;              // A: row m, k; B: k, column m
        const float *xa = X + (16 * m) * Fp + 4 * m + k;
        f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        // the operands of step (f, bg): frame 16 m + s + f of the tile, and the template's frame f - m that column m meets there
        // (in: column m's window holds frame f; the zero above and below the template is selected where the operand is used)
        auto operands = [&](int f, int bg, float &a, float &b, bool &in) {
            const int j = f - m;
            in = (unsigned)j < (unsigned)n;
            a = xa[(f + s) * Fp + 4 * ((f + s) >> 4) + 4 * bg];
            b = T[(in ? j : 0) * FT + k + 4 * bg];
        };
        // every step's operands are read one step ahead of its matrix instruction
        int f = 0, bg = wave;
        float a, b;
        bool in;
        operands(f, bg, a, b, in);
        for (;;) {
            bg += 4;
            if (bg >= groups) {
                bg = wave;
                f++;
            }
            const bool more = f < n + 15;
            float a1 = 0.0f, b1 = 0.0f;
            bool in1 = false;
            if (more) operands(f, bg, a1, b1, in1);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, in ? b : 0.0f, acc, 0, 0, 0);
            if (!more) break;
            a = a1;
            b = b1;
            in = in1;
        }
        for (int r = 0; r < 4; r++) t.red[wave * kMatchTile + 16 * (4 * (lane >> 4) + r) + (lane & 15)] = acc[r];
    }
}

// a thread a position: the waves' sums added in wave order; the window's energy from its first frame on
__device__ __forceinline__ float match_dot(const MatchDesc &d, const MatchTile &t, int tid)
{
    const int groups = d.Fp >> 2, nw = groups < 4 ? groups : 4;
    float dot = t.red[tid];
    for (int w = 1; w < nw; w++) dot = dot + t.red[w * kMatchTile + tid];
    return dot;
}

// (n frames from the staged frame s + tid on)
__device__ __forceinline__ float match_energy(const MatchTile &t, int n, int s, int tid)
{
    float E = 0.0f;
    for (int j = 0; j < n; j++) E = E + t.Efr[tid + s + j];
    return E;
}

__global__ void __launch_bounds__(kThreads)
match_scores_mfma_kernel(MatchDesc d, const float *__restrict__ columns, int64_t n_frames, int64_t row_stride, float *__restrict__ scores)
{
    extern __shared__ float match_lds[];
    const int tid = (int)threadIdx.x, row = (int)blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * kMatchTile;
    const MatchTile t = match_tile(match_lds, d);
    match_stage_frames<false>(d, t, columns + (int64_t)row * row_stride, p0, n_frames, tid);
    match_stage_template(d, t.T, d.templ, d.n, tid);
    __syncthreads();
    match_energies(d, t, tid);
    __syncthreads();
    match_products(d, t, d.n, 0, tid);
    __syncthreads();

    const int64_t q = p0 + tid;
    if (q >= n_frames) return;
    float s = __uint_as_float(0x7fc00000u);
    if (match_position(d, row, q, n_frames)) s = match_score(match_dot(d, t, tid), match_energy(t, d.n, 0, tid));
    scores[(int64_t)row * n_frames + q] = s;
}

// The bank: the frames staged and their energies taken once, then a pass of the same products a template, the templates class by
// class (b.order: ascending k within a class, so a thread holds one running maximum and writes it behind its class's last
// template).  One template region: template i + 1 is staged behind the barrier that ends template i's products, beside the
// thread-a-position step, so K does not enter the tile's LDS.
__global__ void __launch_bounds__(kThreads)
match_bank_scores_mfma_kernel(MatchBankDesc b, const float *__restrict__ columns, int64_t n_frames, int64_t row_stride, float *__restrict__ scores,
                              int32_t *__restrict__ which)
{
    extern __shared__ float match_lds[];
    const MatchDesc &d = b.d;
    const int tid = (int)threadIdx.x, row = (int)blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * kMatchTile;
    const int64_t one = (int64_t)d.n * d.bins;
    const MatchTile t = match_tile(match_lds, d);
    match_stage_frames<false>(d, t, columns + (int64_t)row * row_stride, p0, n_frames, tid);
    match_stage_template(d, t.T, d.templ + b.order[0] * one, d.n, tid);
    __syncthreads();
    match_energies(d, t, tid);
    __syncthreads();

    const int64_t q = p0 + tid;
    const bool live = q < n_frames, pos = live && match_position(d, row, q, n_frames);
    const float E = pos ? match_energy(t, d.n, 0, tid) : 0.0f;    // one sum for the K scores
    const int64_t plane = (int64_t)d.rows * n_frames, at = (int64_t)row * n_frames + q;
    float running;
    int32_t w;
    match_class_begin(running, w);
    for (int i = 0; i < b.K; i++) {
        const int k = b.order[i], c = b.order_class[i];
        const bool more = i + 1 < b.K;
        match_products(d, t, d.n, 0, tid);
        __syncthreads();
        if (more) match_stage_template(d, t.T, d.templ + b.order[i + 1] * one, d.n, tid);
        if (pos) match_class_take(match_score(match_dot(d, t, tid), E), k, running, w);
        if (!more || b.order_class[i + 1] != c) {            // the class's last template
            if (live) {
                scores[c * plane + at] = running;
                if (which) which[c * plane + at] = w;
            }
            match_class_begin(running, w);
        }
        if (more) __syncthreads();                           // (the template and the waves' sums are the next pass's)
    }
}

// The ragged bank: the bank's kernel with a length n_k and an anchor a_k a template (match_ragged.hpp).  Thread tid holds plane
// element u = p0 + tid, the ANCHOR frame; the staged frames begin a_max in front of p0, so template k's window at u, the frames
// [u - a_k, ..), begins at the staged frame tid + s_k, s_k = a_max - a_k.  A pass is the bank's pass with (n_k, s_k); a window's
// energy is summed a template, from the window's first frame on, since the windows differ.  A window exists where it lies inside
// the detector that holds u on both sides: frames in front of the detector only ever meet zeros of the Toeplitz operand.
__global__ void __launch_bounds__(kThreads)
match_ragged_scores_mfma_kernel(MatchRaggedDesc b, const float *__restrict__ columns, int64_t n_frames, int64_t row_stride, float *__restrict__ scores,
                                int32_t *__restrict__ which)
{
    extern __shared__ float match_lds[];
    const MatchDesc &d = b.d;
    const int tid = (int)threadIdx.x, row = (int)blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * kMatchTile;
    const MatchTile t = match_tile_of(match_lds, d, b.G, d.n);
    match_stage_frames<true>(d, t, columns + (int64_t)row * row_stride, p0 - b.a_max, n_frames, tid);
    match_stage_template(d, t.T, d.templ + b.offset[b.order[0]], b.len[b.order[0]], tid);
    __syncthreads();
    match_energies(d, t, tid);
    __syncthreads();

    const int64_t q = p0 + tid;
    const bool live = q < n_frames;
    int64_t first = 0, end = 0;
    const bool held = live && match_holder(d, row, q, n_frames, first, end);
    const int64_t plane = (int64_t)d.rows * n_frames, at = (int64_t)row * n_frames + q;
    float running;
    int32_t w;
    match_class_begin(running, w);
    for (int i = 0; i < b.K; i++) {
        const int k = b.order[i], c = b.order_class[i];
        const int n = b.len[k], a = b.anchor[k], s = b.a_max - a;
        const bool more = i + 1 < b.K;
        match_products(d, t, n, s, tid);
        __syncthreads();
        if (more) match_stage_template(d, t.T, d.templ + b.offset[b.order[i + 1]], b.len[b.order[i + 1]], tid);
        if (held && match_ragged_window(first, end, q, a, n)) match_class_take(match_score(match_dot(d, t, tid), match_energy(t, n, s, tid)), k, running, w);
        if (!more || b.order_class[i + 1] != c) {            // the class's last template
            if (live) {
                scores[c * plane + at] = running;
                if (which) which[c * plane + at] = w;
            }
            match_class_begin(running, w);
        }
        if (more) __syncthreads();                           // (the template and the waves' sums are the next pass's)
    }
}

// one thread a position: the window's chains from global memory
template <bool kEnergy>
__device__ __forceinline__ void match_plain_chains(const float *__restrict__ x, const float *__restrict__ t, int n, int bins, float &dot, float &E)
{
    dot = 0.0f;
    if (kEnergy) E = 0.0f;
    for (int j = 0; j < n; j++) {
        float e = 0.0f;
        for (int b = 0; b < bins; b++) {
            const float v = x[j * bins + b];
            if (kEnergy) e = fmaf(v, v, e);
            dot = fmaf(finite_bits(v) ? v : 0.0f, t[j * bins + b], dot);
        }
        if (kEnergy) E = E + e;
    }
}

__global__ void __launch_bounds__(kThreads)
match_scores_plain_kernel(MatchDesc d, const float *__restrict__ columns, int64_t n_frames, int64_t row_stride, float *__restrict__ scores)
{
    const int row = (int)blockIdx.y;
    const int64_t q = (int64_t)blockIdx.x * kMatchTile + (int)threadIdx.x;
    if (q >= n_frames) return;
    float s = __uint_as_float(0x7fc00000u);
    if (match_position(d, row, q, n_frames)) {
        float dot, E;
        match_plain_chains<true>(columns + (int64_t)row * row_stride + q * d.bins, d.templ, d.n, d.bins, dot, E);
        s = match_score(dot, E);
    }
    scores[(int64_t)row * n_frames + q] = s;
}

// the bank: the same chains a template, E with the first
__global__ void __launch_bounds__(kThreads)
match_bank_scores_plain_kernel(MatchBankDesc b, const float *__restrict__ columns, int64_t n_frames, int64_t row_stride, float *__restrict__ scores,
                               int32_t *__restrict__ which)
{
    const MatchDesc &d = b.d;
    const int row = (int)blockIdx.y;
    const int64_t q = (int64_t)blockIdx.x * kMatchTile + (int)threadIdx.x;
    if (q >= n_frames) return;
    const bool pos = match_position(d, row, q, n_frames);
    const float *__restrict__ x = columns + (int64_t)row * row_stride + q * d.bins;
    const int64_t one = (int64_t)d.n * d.bins, plane = (int64_t)d.rows * n_frames, at = (int64_t)row * n_frames + q;
    float running, E = 0.0f;
    int32_t w;
    match_class_begin(running, w);
    for (int i = 0; i < b.K; i++) {
        const int k = b.order[i], c = b.order_class[i];
        if (pos) {
            float dot;
            if (i == 0) match_plain_chains<true>(x, d.templ + k * one, d.n, d.bins, dot, E);
            else match_plain_chains<false>(x, d.templ + k * one, d.n, d.bins, dot, E);
            match_class_take(match_score(dot, E), k, running, w);
        }
        if (i + 1 == b.K || b.order_class[i + 1] != c) {
            scores[c * plane + at] = running;
            if (which) which[c * plane + at] = w;
            match_class_begin(running, w);
        }
    }
}

// the ragged bank: a thread a plane element, the chains of template k's window from its first frame u - a_k on, E a template
__global__ void __launch_bounds__(kThreads)
match_ragged_scores_plain_kernel(MatchRaggedDesc b, const float *__restrict__ columns, int64_t n_frames, int64_t row_stride, float *__restrict__ scores,
                                 int32_t *__restrict__ which)
{
    const MatchDesc &d = b.d;
    const int row = (int)blockIdx.y;
    const int64_t q = (int64_t)blockIdx.x * kMatchTile + (int)threadIdx.x;
    if (q >= n_frames) return;
    int64_t first = 0, end = 0;
    const bool held = match_holder(d, row, q, n_frames, first, end);
    const float *__restrict__ x = columns + (int64_t)row * row_stride;
    const int64_t plane = (int64_t)d.rows * n_frames, at = (int64_t)row * n_frames + q;
    float running;
    int32_t w;
    match_class_begin(running, w);
    for (int i = 0; i < b.K; i++) {
        const int k = b.order[i], c = b.order_class[i];
        const int n = b.len[k], a = b.anchor[k];
        if (held && match_ragged_window(first, end, q, a, n)) {
            float dot, E;
            match_plain_chains<true>(x + (q - a) * d.bins, d.templ + b.offset[k], n, d.bins, dot, E);
            match_class_take(match_score(dot, E), k, running, w);
        }
        if (i + 1 == b.K || b.order_class[i + 1] != c) {
            scores[c * plane + at] = running;
            if (which) which[c * plane + at] = w;
            match_class_begin(running, w);
        }
    }
}

// One detector's matches among the scores of its plane: the body of match_peaks_kernel and, a class a block row, of
// match_bank_peaks_kernel (which, event_template: the bank's, nullptr otherwise).
__device__ __forceinline__ void match_peaks_body(const MatchDesc &d, const float *__restrict__ scores, const int32_t *__restrict__ which, int64_t n_frames,
                                                 uint32_t threshold_key, int S, int64_t *__restrict__ events, int64_t capacity,
                                                 int64_t *__restrict__ counts, float *__restrict__ event_scores, int32_t *__restrict__ event_template,
                                                 uint32_t *match_keys, int *wave_sum)
{
    const int tid = (int)threadIdx.x, det = (int)blockIdx.x;
    int64_t row = det, first = 0, U = n_frames;
    if (d.by_det) {
        const DetSpan e = d.by_det[det];
        row = e.row;
        first = e.first;
        U = e.units;
    }
    const int64_t P = U - d.n + 1;                           // the detector's positions
    const int L = kMatchChunk + 2 * S, k = S ? match_level(S) : 0;
    const float *__restrict__ s = scores + row * n_frames + first;
    int64_t total = 0;
    for (int64_t c0 = 0; c0 < P; c0 += kMatchChunk) {
        uint32_t *cur = match_keys, *nxt = match_keys + L;
        for (int i = tid; i < L; i += kThreads) {
            const int64_t q = c0 - S + i;
            cur[i] = q >= 0 && q < P ? match_key(s[q]) : 0u;
        }
        __syncthreads();
        uint32_t key[kOwn];
        for (int e = 0; e < kOwn; e++) key[e] = cur[S + tid * kOwn + e];
        for (int lev = 0; lev < k; lev++) {                  // cur[i]: the largest key of [i, i + 2^lev)
            const int h = 1 << lev;
            for (int i = tid; i < L; i += kThreads) {
                const uint32_t a = cur[i], b = i + h < L ? cur[i + h] : 0u;
                nxt[i] = a > b ? a : b;
            }
            __syncthreads();
            uint32_t *t = cur;
            cur = nxt;
            nxt = t;
        }
        unsigned flags = 0;
        for (int e = 0; e < kOwn; e++) {
            const int i = S + tid * kOwn + e;
            if (c0 + tid * kOwn + e < P && match_rule(key[e], match_left(cur, i, S, k), match_right(cur, i, S, k), threshold_key)) flags |= 1u << e;
        }
        // the workgroup's matches in front of this thread's
        const int mine = __popc(flags);
        int incl = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o);
            if ((tid & 63) >= o) incl += up;
        }
        if ((tid & 63) == 63) wave_sum[tid >> 6] = incl;
        __syncthreads();
        int before = incl - mine, all = 0;
        for (int w = 0; w < kThreads / 64; w++) {
            if (w < (tid >> 6)) before += wave_sum[w];
            all += wave_sum[w];
        }
        int64_t at = total + before;
        for (int e = 0; e < kOwn; e++) {
            if (!((flags >> e) & 1u)) continue;
            const int64_t p = c0 + tid * kOwn + e;
            if (at < capacity) {
                events[(int64_t)det * capacity + at] = match_event(d.origin, d.hop, p, d.anchor);
                if (event_scores) event_scores[(int64_t)det * capacity + at] = s[p];
                if (event_template) event_template[(int64_t)det * capacity + at] = which[row * n_frames + first + p];
            }
            at++;
        }
        total += all;
        __syncthreads();                                     // (the keys and wave_sum are the next step's)
    }
    if (tid == 0) counts[det] = total;
}

__global__ void __launch_bounds__(kThreads)
match_peaks_kernel(MatchDesc d, const float *__restrict__ scores, int64_t n_frames, uint32_t threshold_key, int S, int64_t *__restrict__ events,
                   int64_t capacity, int64_t *__restrict__ counts, float *__restrict__ event_scores)
{
    extern __shared__ uint32_t match_keys[];
    __shared__ int wave_sum[kThreads / 64];
    match_peaks_body(d, scores, nullptr, n_frames, threshold_key, S, events, capacity, counts, event_scores, nullptr, match_keys, wave_sum);
}

// grid (D, C): class c's plane with class c's threshold into class c's tables; classes do not meet
__global__ void __launch_bounds__(kThreads)
match_bank_peaks_kernel(MatchBankDesc b, MatchBankKeys keys, const float *__restrict__ scores, const int32_t *__restrict__ which, int64_t n_frames, int S,
                        int64_t *__restrict__ events, int64_t capacity, int64_t *__restrict__ counts, float *__restrict__ event_scores,
                        int32_t *__restrict__ event_template)
{
    extern __shared__ uint32_t match_keys[];
    __shared__ int wave_sum[kThreads / 64];
    const int c = (int)blockIdx.y;
    uint32_t key = 0u;
#pragma unroll
    for (int e = 0; e < kMatchMaxClasses; e++)
        if (e == c) key = keys.key[e];
    const int64_t plane = (int64_t)b.d.rows * n_frames, table = (int64_t)b.d.D * capacity;
    match_peaks_body(b.d, scores + c * plane, which ? which + c * plane : nullptr, n_frames, key, S, events + c * table, capacity,
                     counts + (int64_t)c * b.d.D, event_scores ? event_scores + c * table : nullptr,
                     event_template ? event_template + c * table : nullptr, match_keys, wave_sum);
}

// ... with class c's own separation beside its key (a short syllable repeats faster than a long one)
__global__ void __launch_bounds__(kThreads)
match_bank_peaks_each_kernel(MatchBankDesc b, MatchBankKeys keys, MatchBankSeps seps, const float *__restrict__ scores, const int32_t *__restrict__ which,
                             int64_t n_frames, int64_t *__restrict__ events, int64_t capacity, int64_t *__restrict__ counts,
                             float *__restrict__ event_scores, int32_t *__restrict__ event_template)
{
    extern __shared__ uint32_t match_keys[];
    __shared__ int wave_sum[kThreads / 64];
    const int c = (int)blockIdx.y;
    uint32_t key = 0u;
    int S = 0;
#pragma unroll
    for (int e = 0; e < kMatchMaxClasses; e++)
        if (e == c) {
            key = keys.key[e];
            S = seps.S[e];
        }
    const int64_t plane = (int64_t)b.d.rows * n_frames, table = (int64_t)b.d.D * capacity;
    match_peaks_body(b.d, scores + c * plane, which ? which + c * plane : nullptr, n_frames, key, S, events + c * table, capacity,
                     counts + (int64_t)c * b.d.D, event_scores ? event_scores + c * table : nullptr,
                     event_template ? event_template + c * table : nullptr, match_keys, wave_sum);
}

}  // namespace

void match_plan(MatchDesc &d)
{
    const int64_t G = kMatchTile - 1 + d.n;
    const int64_t floats = match_tile_floats(G, d.n, d.bins, &d.Fp, &d.FT);
    d.matrix = floats * 4 <= kMatchLdsBytes;
    d.lds_bytes = d.matrix ? (int)(floats * 4) : 0;
}

hipError_t match_prepare()
{
    return hipFuncSetAttribute((const void *)match_peaks_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               2 * (kMatchChunk + 2 * kMatchMaxSeparation) * (int)sizeof(uint32_t));
}

hipError_t launch_match_scores(const MatchDesc &d, const float *columns, int64_t n_frames, int64_t row_stride, float *scores, hipStream_t stream)
{
    if (n_frames <= 0 || d.rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n_frames + kMatchTile - 1) / kMatchTile), (unsigned)d.rows);
    if (d.matrix)
        hipLaunchKernelGGL(match_scores_mfma_kernel, grid, dim3(kThreads), (size_t)d.lds_bytes, stream, d, columns, n_frames, row_stride, scores);
    else
        hipLaunchKernelGGL(match_scores_plain_kernel, grid, dim3(kThreads), 0, stream, d, columns, n_frames, row_stride, scores);
    return hipGetLastError();
}

hipError_t launch_match_peaks(const MatchDesc &d, const float *scores, int64_t n_frames, float threshold, int separation, int64_t *events,
                              int64_t capacity, int64_t *counts, float *event_scores, hipStream_t stream)
{
    if (d.D <= 0) return hipSuccess;
    const size_t lds = 2 * (size_t)(kMatchChunk + 2 * separation) * sizeof(uint32_t);
    hipLaunchKernelGGL(match_peaks_kernel, dim3((unsigned)d.D), dim3(kThreads), lds, stream, d, scores, n_frames, match_key(threshold), separation,
                       events, capacity, counts, event_scores);
    return hipGetLastError();
}

hipError_t match_bank_prepare()
{
    const int lds = 2 * (kMatchChunk + 2 * kMatchMaxSeparation) * (int)sizeof(uint32_t);
    if (hipError_t e = hipFuncSetAttribute((const void *)match_bank_peaks_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds)) return e;
    return hipFuncSetAttribute((const void *)match_bank_peaks_each_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
}

hipError_t launch_match_bank_scores(const MatchBankDesc &b, const float *columns, int64_t n_frames, int64_t row_stride, float *scores, int32_t *which,
                                    hipStream_t stream)
{
    if (n_frames <= 0 || b.d.rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n_frames + kMatchTile - 1) / kMatchTile), (unsigned)b.d.rows);
    if (b.d.matrix)
        hipLaunchKernelGGL(match_bank_scores_mfma_kernel, grid, dim3(kThreads), (size_t)b.d.lds_bytes, stream, b, columns, n_frames, row_stride, scores,
                           which);
    else
        hipLaunchKernelGGL(match_bank_scores_plain_kernel, grid, dim3(kThreads), 0, stream, b, columns, n_frames, row_stride, scores, which);
    return hipGetLastError();
}

hipError_t launch_match_bank_peaks(const MatchBankDesc &b, const float *scores, const int32_t *which, int64_t n_frames, const float *thresholds,
                                   int separation, int64_t *events, int64_t capacity, int64_t *counts, float *event_scores, int32_t *event_template,
                                   hipStream_t stream)
{
    if (b.d.D <= 0) return hipSuccess;
    MatchBankKeys keys{};
    for (int c = 0; c < b.C; c++) keys.key[c] = match_key(thresholds[c]);
    const size_t lds = 2 * (size_t)(kMatchChunk + 2 * separation) * sizeof(uint32_t);
    hipLaunchKernelGGL(match_bank_peaks_kernel, dim3((unsigned)b.d.D, (unsigned)b.C), dim3(kThreads), lds, stream, b, keys, scores, which, n_frames,
                       separation, events, capacity, counts, event_scores, event_template);
    return hipGetLastError();
}

hipError_t launch_match_bank_peaks_each(const MatchBankDesc &b, const float *scores, const int32_t *which, int64_t n_frames, const float *thresholds,
                                        const int32_t *separations, int64_t *events, int64_t capacity, int64_t *counts, float *event_scores,
                                        int32_t *event_template, hipStream_t stream)
{
    if (b.d.D <= 0) return hipSuccess;
    MatchBankKeys keys{};
    MatchBankSeps seps{};
    int most = 0;
    for (int c = 0; c < b.C; c++) {
        keys.key[c] = match_key(thresholds[c]);
        seps.S[c] = separations[c];
        most = separations[c] > most ? separations[c] : most;
    }
    const size_t lds = 2 * (size_t)(kMatchChunk + 2 * most) * sizeof(uint32_t);
    hipLaunchKernelGGL(match_bank_peaks_each_kernel, dim3((unsigned)b.d.D, (unsigned)b.C), dim3(kThreads), lds, stream, b, keys, seps, scores, which,
                       n_frames, events, capacity, counts, event_scores, event_template);
    return hipGetLastError();
}

hipError_t launch_match_ragged_scores(const MatchRaggedDesc &b, const float *columns, int64_t n_frames, int64_t row_stride, float *scores,
                                      int32_t *which, hipStream_t stream)
{
    if (n_frames <= 0 || b.d.rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n_frames + kMatchTile - 1) / kMatchTile), (unsigned)b.d.rows);
    if (b.d.matrix)
        hipLaunchKernelGGL(match_ragged_scores_mfma_kernel, grid, dim3(kThreads), (size_t)b.d.lds_bytes, stream, b, columns, n_frames, row_stride, scores,
                           which);
    else
        hipLaunchKernelGGL(match_ragged_scores_plain_kernel, grid, dim3(kThreads), 0, stream, b, columns, n_frames, row_stride, scores, which);
    return hipGetLastError();
}

}  // namespace sd
