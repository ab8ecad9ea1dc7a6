// syldet_api.cpp -- the handle's life-cycle (create / create_multi / create_mixed / destroy), table upload, the choice of the
// engine, the geometry and profile getters.  The batch calls are syldet_run.cpp's, the streaming front end syldet_stream.cpp's.
//
// There is no CPU execution path in this library: every entry point that computes runs
// HIP kernels on a gfx950 device, and create fails without one.

#include "syldet_handle.hpp"

namespace {

const char kFixupName[] = "fixup_kernel";   // the exact recomputation in syldet_timings (timed_fixup, syldet_run.cpp)

// The generic engine's parameter blob of one network (NetDesc's offsets point into it) and the NetDesc that describes it;
// compatible networks give the same offsets and the same blob length.
int make_net_blob(const syldet_config_t &c, const syldet_geometry_t &g, NetDesc &n, std::vector<float> &blob)
{
    std::memset(&n, 0, sizeof(n));
    blob.clear();
    if (c.n_input_fns > kMaxFns || c.n_output_fns > kMaxFns || c.n_layers > kMaxLayers)
        return fail(SYLDET_ERR_UNSUPPORTED, "more than 8 processing functions or 8 layers");
    auto push = [&blob](const float *p, size_t cnt) {
        const int off = (int)blob.size();
        blob.insert(blob.end(), p, p + cnt);
        return off;
    };
    n.n_in_fns = c.n_input_fns;
    for (int i = 0; i < c.n_input_fns; i++) {
        const syldet_fn_t &f = c.input_fns[i];
        n.in_fns[i].kind = f.kind;
        n.in_fns[i].y = f.y;
        n.in_fns[i].yoff = push(&f.y, 1);
        if (f.count > 0) {
            n.in_fns[i].xoff = push(f.x_offsets, (size_t)f.count);
            n.in_fns[i].gain = push(f.gains, (size_t)f.count);
        }
    }
    n.n_layers = c.n_layers;
    int max_width = g.inputs;
    for (int l = 0; l < c.n_layers; l++) {
        const syldet_layer_t &L = c.layers[l];
        n.layers[l].in = L.inputs;
        n.layers[l].out = L.outputs;
        n.layers[l].tf = L.transfer;
        n.layers[l].w = push(L.weights, (size_t)L.inputs * (size_t)L.outputs);
        n.layers[l].b = push(L.biases, (size_t)L.outputs);
        max_width = std::max(max_width, L.outputs);
    }
    n.n_out_fns = c.n_output_fns;
    for (int i = 0; i < c.n_output_fns; i++) {
        const syldet_fn_t &f = c.output_fns[i];
        n.out_fns[i].kind = f.kind;
        n.out_fns[i].y = f.y;
        n.out_fns[i].yoff = push(&f.y, 1);
        n.out_fns[i].xoff = push(f.x_offsets, (size_t)f.count);
        n.out_fns[i].gain = push(f.gains, (size_t)f.count);
    }
    n.I = g.inputs;
    n.n_out = g.outputs;
    n.max_width = max_width;
    n.scaling = c.scaling;
    n.rule = c.rule;
    if ((size_t)max_width * 2 * 4 * sizeof(float) > 160 * 1024)
        return fail(SYLDET_ERR_UNSUPPORTED, "layer wider than the generic engine's LDS budget");
    return SYLDET_OK;
}

int build_tables(syldet *h)
{
    const syldet_config_t &c = h->cfg.view;
    const syldet_geometry_t &g = h->geom;
    const int N = c.fourier_length, W = c.window_length, M = N / 2;
    int logM = 0;
    while ((1 << logM) < M) logM++;

    std::vector<float> win((size_t)W);
    make_window(c.window, W, win.data());
    std::vector<float2> tw((size_t)std::max(1, M / 2)), sw((size_t)M);
    const double two_pi = 6.283185307179586476925286766559;
    for (int t = 0; t < M / 2; t++) {
        const double a = -two_pi * (double)t / (double)M;
        tw[(size_t)t] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    for (int k = 0; k < M; k++) {
        const double a = -two_pi * (double)k / (double)N;
        sw[(size_t)k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    if (int st = h->d_window.reserve(win.size() * sizeof(float))) return st;
    if (int st = h->d_tw.reserve(tw.size() * sizeof(float2))) return st;
    if (int st = h->d_sw.reserve(sw.size() * sizeof(float2))) return st;
    SYLDET_HIP(hipMemcpy(h->d_window.ptr, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice));
    SYLDET_HIP(hipMemcpy(h->d_tw.ptr, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice));
    SYLDET_HIP(hipMemcpy(h->d_sw.ptr, sw.data(), sw.size() * sizeof(float2), hipMemcpyHostToDevice));

    StftDesc &s = h->stft;
    s.N = N; s.W = W; s.M = M; s.logM = logM;
    s.hop = g.hop; s.gap = g.gap; s.f0 = g.f0; s.F = g.bins;
    s.power_mode = c.spectrum == SYLDET_SPECTRUM_MAGNITUDE ? 1 : 0;
    s.window = (const float *)h->d_window.ptr;
    s.tw = (const float2 *)h->d_tw.ptr;
    s.sw = (const float2 *)h->d_sw.ptr;

    // parameter blob for the unfolded network
    NetDesc &n = h->net;
    std::vector<float> blob;
    if (int st = make_net_blob(c, g, n, blob)) return st;
    if (int st = h->d_params.reserve(std::max<size_t>(blob.size(), 1) * sizeof(float))) return st;
    if (!blob.empty())
        SYLDET_HIP(hipMemcpy(h->d_params.ptr, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice));
    if (int st = h->d_thr.reserve((size_t)c.n_thresholds * sizeof(double))) return st;
    SYLDET_HIP(hipMemcpy(h->d_thr.ptr, c.thresholds, (size_t)c.n_thresholds * sizeof(double), hipMemcpyHostToDevice));
    n.params = (const float *)h->d_params.ptr;
    n.thresholds = (const double *)h->d_thr.ptr;
    return SYLDET_OK;
}

// float -> bf16, round to nearest even (what v_cvt_pk_bf16_f32 does on the device)
uint16_t to_bf16(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// Wide-network engine tables: the first layer in MFMA A-operand order, 32 hidden units per chunk (kernels_wide.hip).
int upload_wide(syldet *h, std::string &why)
{
    const syldet_config_t &c = h->cfg.view;
    if (c.n_layers != 2) { why = "needs exactly two layers"; return SYLDET_ERR_UNSUPPORTED; }
    const syldet_layer_t &L0 = c.layers[0], &L1 = c.layers[1];
    if (L0.inputs > kWideK) { why = "more than 320 network inputs"; return SYLDET_ERR_UNSUPPORTED; }
    if (L0.outputs < 32) { why = "hidden layer narrower than 32 units"; return SYLDET_ERR_UNSUPPORTED; }
    if (L1.outputs > 4) { why = "more than 4 outputs"; return SYLDET_ERR_UNSUPPORTED; }
    const int I = L0.inputs, H = L0.outputs, n_out = L1.outputs, n_chunks = (H + 31) / 32;
    const size_t chunk_u16 = kWideChunkBytes / 2;
    std::vector<uint16_t> pack((size_t)n_chunks * chunk_u16, 0);
    // TanSig / LogSig hidden layers are folded into the tables: tanh(x) = 1 - 2 / (2^(s x) + 1) with s = 2 log2(e),
    // logsig(x) = 1 / (2^(s x) + 1) with s = -log2(e).  The kernel then computes r = 1 / (2^acc + 1) with acc = s (W0 x + b0)
    // and y += w1' r, where w1' = -2 w1 and b1' = b1 + sum w1 for tanh, unchanged for logsig.
    const bool sig = L0.transfer == SYLDET_TF_TANSIG || L0.transfer == SYLDET_TF_LOGSIG;
    const bool shape16 = !h->sw.wide_shape32;
    // The input chain the training script writes -- [l2normalize,] affine maps, on linear columns -- needs no preparation pass:
    // u_i = a_i (v_i r) + o_i with r = 1 / |v| (or 1), so W0 u + b0 = (W0 diag a) (v r) + (W0 o + b0): the affine part goes
    // into the first layer here, and the GEMM kernel makes its operands bf16(v r) from the columns themselves.  (Also the
    // better numbers: bf16 keeps 8 bits of v r instead of 8 bits of a value that sits next to -1.)
    bool front = shape16 && !h->sw.wide_no_front && c.scaling == SYLDET_SCALING_LINEAR && wide_front_fits(h->geom.bins, I);
    int l2 = 0;
    std::vector<double> fa((size_t)I, 1.0), fo((size_t)I, 0.0);
    for (int k = 0; k < c.n_input_fns && front; k++) {
        const syldet_fn_t &f = c.input_fns[k];
        if (f.kind == SYLDET_FN_L2NORMALIZE && k == 0) { l2 = 1; continue; }
        if (f.kind != SYLDET_FN_MAPMINMAX && f.kind != SYLDET_FN_MAPSTD) { front = false; break; }
        for (int i = 0; i < I; i++) {                              // MapMinMax.apply :127-131, MapStd.apply :162-169
            fo[(size_t)i] = (fo[(size_t)i] - (double)f.x_offsets[i]) * (double)f.gains[i] + (double)f.y;
            fa[(size_t)i] *= (double)f.gains[i];
        }
    }
    // The fold quantises v r (not u = a v r + o) to bf16: an error of 2^-9 |a_i v_i r| in u_i.  For maps trained on a range
    // around zero (the example net: offsets of 1e-5, gains of 4) that is the better deal; for a range away from zero
    // (x in [0.05, 0.06]: |a x| = 11 against |u| <= 1) the same relative error is |o_i| times larger in u than bf16(u) would
    // leave, and the 1e-2 bar goes.  |o_i| = |u_i - a_i v_i r| bounds |a_i v_i r| wherever u is O(1): such chains keep the
    // preparation kernel, which rounds u itself.
    if (front) {
        double worst = 0.0;
        for (int i = 0; i < I; i++) worst = std::max(worst, std::fabs(fo[(size_t)i]));
        if (!(worst <= 4.0)) front = false;
    }
    // SYLDET_WIDE_TANH_POLY (round 6, an A/B form): the kernel evaluates t = tanh_poly(acc) -- a clamped odd polynomial, no
    // transcendental -- and y += w1' t.  tanh: acc = W0 x + b0, w1' = w1; logsig(x) = 1/2 + tanh(x / 2) / 2: acc = (W0 x + b0) / 2,
    // w1' = w1 / 2, b1' = b1 + sum w1 / 2.
    // SYLDET_WIDE_M32: the chunks in the 32x32x16 order for wide_gemm32s_kernel (one output, the front end, 256 evaluations' columns
    // and two chunk buffers in half a CU's LDS: launch_wide_gemm checks the same)
    // (a band too wide for that keeps the 16x16x32 kernel under the switch, as a network of several outputs does: the launch
    // would refuse it)
    const bool m32 = shape16 && front && n_out == 1 && h->sw.wide_m32 && !h->sw.wide_tanh_poly && wide_front_fits_half(h->geom.bins, I);
    const bool pack16 = shape16 && !m32;
    const bool poly = sig && shape16 && front && n_out == 1 && h->sw.wide_tanh_poly;   // (the forms that have an instantiation: kernels_wide.hip)
    const double sc = !sig ? 1.0 : poly ? (L0.transfer == SYLDET_TF_TANSIG ? 1.0 : 0.5)
                                        : (L0.transfer == SYLDET_TF_TANSIG ? 2.8853900817779268 : -1.4426950408889634);
    const double w1s = !sig ? 1.0 : poly ? (L0.transfer == SYLDET_TF_TANSIG ? 1.0 : 0.5) : (L0.transfer == SYLDET_TF_TANSIG ? -2.0 : 1.0);
    for (int ch = 0; ch < n_chunks; ch++) {
        uint16_t *frag = pack.data() + (size_t)ch * chunk_u16;
        for (int ks = 0; ks < kWideK / 16; ks++)
            for (int l = 0; l < 64; l++)
                for (int j = 0; j < 8; j++) {
                    // 32x32x16: fragment ks = k-step of 16, lane l = unit l % 32, k = 8 (l / 32) + j
                    // 16x16x32: fragment ks = (k-step of 32, unit tile of 16), lane l = unit l % 16 of its tile, k = 8 (l / 16) + j
                    const int unit = pack16 ? 32 * ch + 16 * (ks & 1) + (l & 15) : 32 * ch + (l & 31);
                    const int k = pack16 ? 32 * (ks >> 1) + 8 * (l >> 4) + j : 16 * ks + 8 * (l >> 5) + j;
                    const float v = (unit < H && k < I) ? (float)(sc * (double)L0.weights[(size_t)unit * I + k] * (front ? fa[(size_t)k] : 1.0)) : 0.0f;
                    frag[((size_t)ks * 64 + l) * 8 + j] = to_bf16(v);
                }
        float *cst = reinterpret_cast<float *>(frag + (size_t)(kWideK / 16) * 64 * 8);
        for (int u = 0; u < 32; u++) {
            const int unit = 32 * ch + u;
            double b0f = unit < H ? (double)L0.biases[unit] : 0.0;
            if (front && unit < H)
                for (int i = 0; i < I; i++) b0f += (double)L0.weights[(size_t)unit * I + i] * fo[(size_t)i];
            cst[u] = unit < H ? (float)(sc * b0f) : 0.0f;
            for (int o = 0; o < 4; o++) cst[32 + 32 * o + u] = (unit < H && o < n_out) ? (float)(w1s * (double)L1.weights[(size_t)o * H + unit]) : 0.0f;
        }
    }
    std::vector<float> misc((size_t)n_out);
    for (int o = 0; o < n_out; o++) {
        double b = (double)L1.biases[o];
        if (sig && !poly && L0.transfer == SYLDET_TF_TANSIG)
            for (int u = 0; u < H; u++) b += (double)L1.weights[(size_t)o * H + u];
        if (poly && L0.transfer == SYLDET_TF_LOGSIG)
            for (int u = 0; u < H; u++) b += 0.5 * (double)L1.weights[(size_t)o * H + u];
        misc[(size_t)o] = (float)b;
    }
    for (int k = 0; k < c.n_output_fns; k++) {
        const syldet_fn_t &f = c.output_fns[k];
        misc.push_back(f.y);
        misc.insert(misc.end(), f.gains, f.gains + n_out);
        misc.insert(misc.end(), f.x_offsets, f.x_offsets + n_out);
    }
    const size_t pack_bytes = pack.size() * 2, misc_bytes = misc.size() * sizeof(float);
    if (int st = h->d_wide.reserve(pack_bytes + misc_bytes)) return st;
    SYLDET_HIP(hipMemcpy(h->d_wide.ptr, pack.data(), pack_bytes, hipMemcpyHostToDevice));
    SYLDET_HIP(hipMemcpy((char *)h->d_wide.ptr + pack_bytes, misc.data(), misc_bytes, hipMemcpyHostToDevice));
    WideDesc &d = h->wide;
    d.H = H; d.n_chunks = n_chunks; d.n_out = n_out; d.tf0 = L0.transfer; d.tf1 = L1.transfer; d.rule = c.rule;
    d.n_out_fns = c.n_output_fns;
    d.sig = sig ? 1 : 0;
    d.poly = poly ? 1 : 0;
    d.m32 = m32 ? 1 : 0;
    d.shape16 = shape16 ? 1 : 0;
    d.front = front ? 1 : 0; d.l2 = l2; d.I = I; d.F = h->geom.bins;
    d.wg8 = h->sw.wide_wg16 ? 0 : 1;
    d.stagger = h->sw.wide_stagger ? 1 : 0;
    d.dma_builtin = h->sw.wide_dma_builtin ? 1 : 0;
    d.tiles4 = h->sw.wide_tiles4 ? 1 : 0;
    d.wpack = (const uint4 *)h->d_wide.ptr;
    d.b1 = (const float *)((const char *)h->d_wide.ptr + pack_bytes);
    d.out_params = d.b1 + n_out;
    d.thresholds = (const double *)h->d_thr.ptr;
    return SYLDET_OK;
}

int upload_plan(syldet *h, FusedPlan &p, DeviceBuffer &buf)
{
    std::vector<unsigned char> blob;
    auto put = [&blob](const void *src, size_t bytes) {
        const size_t off = (blob.size() + 255) / 256 * 256;
        blob.resize(off + std::max<size_t>(bytes, 16));
        if (bytes) std::memcpy(blob.data() + off, src, bytes);
        return off;
    };
    const size_t o_d = put(p.dfrag.data(), p.dfrag.size() * 2), o_w = put(p.afrag.data(), p.afrag.size() * 2);
    const size_t o_k = put(p.koff.data(), p.koff.size() * 4), o_b = put(p.bias0.data(), p.bias0.size() * 4);
    const size_t o_r = put(p.rvec.data(), p.rvec.size() * 4), o_w1 = put(p.w1.data(), p.w1.size() * 4);
    const size_t o_b1 = put(p.b1.data(), p.b1.size() * 4), o_op = put(p.out_params.data(), p.out_params.size() * 4);
    const size_t o_wt = put(p.afrag_t.data(), p.afrag_t.size() * 2);
    const size_t o_sf = put(p.sfrag.data(), p.sfrag.size() * 2), o_sl = put(p.slone.data(), p.slone.size() * 4);
    const size_t o_ww = put(p.afrag_w.data(), p.afrag_w.size() * 2);
    const size_t o_s2 = put(p.sfrag2.data(), p.sfrag2.size() * 2), o_w2 = put(p.swin2.data(), p.swin2.size() * 4);
    const size_t o_c2 = put(p.s2c.data(), p.s2c.size() * 4), o_t2 = put(p.afrag_t2.data(), p.afrag_t2.size() * 2);
    const size_t o_x2 = put(p.afrag_w2.data(), p.afrag_w2.size() * 2);
    if (int st = buf.reserve(blob.size())) return st;
    SYLDET_HIP(hipMemcpy(buf.ptr, blob.data(), blob.size(), hipMemcpyHostToDevice));
    unsigned char *base = (unsigned char *)buf.ptr;
    FusedDesc &d = p.desc;
    d.dfrag = (const uint4 *)(base + o_d);
    d.afrag = (const uint4 *)(base + o_w);
    d.afrag_t = (const uint4 *)(base + o_wt);
    d.sfrag = (const uint4 *)(base + o_sf);
    d.slone = (const float *)(base + o_sl);
    d.afrag_w = (const uint4 *)(base + o_ww);
    d.sfrag2 = (const uint4 *)(base + o_s2);
    d.swin2 = (const float *)(base + o_w2);
    d.s2c = (const float *)(base + o_c2);
    d.afrag_t2 = (const uint4 *)(base + o_t2);
    d.afrag_w2 = (const uint4 *)(base + o_x2);
    d.koff = (const int *)(base + o_k);
    d.bias0 = (const float *)(base + o_b);
    d.rvec = (const float *)(base + o_r);
    d.w1 = (const float *)(base + o_w1);
    d.b1 = (const float *)(base + o_b1);
    d.out_params = (const float *)(base + o_op);
    d.thresholds = (const double *)h->d_thr.ptr;
    return SYLDET_OK;
}

int upload_fused(syldet *h) { return upload_plan(h, h->fused, h->d_fused); }

// What fixup_kernel (the exact recomputation behind the fused kernels' precision guard) needs: geometry, the fp32 window
// table, a trigonometric table in fp64.
int upload_fix(syldet *h)
{
    const syldet_config_t &c = h->cfg.view;
    const int N = c.fourier_length;
    std::vector<double> tab((size_t)N * 2);
    const double two_pi = 6.283185307179586476925286766559;
    for (int m = 0; m < N; m++) {
        tab[(size_t)2 * m] = std::cos(two_pi * (double)m / (double)N);
        tab[(size_t)2 * m + 1] = std::sin(two_pi * (double)m / (double)N);
    }
    if (int st = h->d_ctab.reserve(tab.size() * sizeof(double))) return st;
    SYLDET_HIP(hipMemcpy(h->d_ctab.ptr, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    FixDesc &f = h->fixd;
    f.N = N; f.W = c.window_length; f.hop = h->geom.hop; f.gap = h->geom.gap; f.f0 = h->geom.f0; f.F = h->geom.bins; f.T = c.time_range;
    f.power_mode = c.spectrum == SYLDET_SPECTRUM_MAGNITUDE ? 1 : 0;
    f.window = (const float *)h->d_window.ptr;
    f.ctab = (const double2 *)h->d_ctab.ptr;
    h->has_fix = true;
    return SYLDET_OK;
}

int upload_mlpx(syldet *h)
{
    MlpxPlan &p = h->mlpx;
    const size_t a_bytes = (p.afrag.size() * 2 + 255) / 256 * 256;
    std::vector<unsigned char> blob(a_bytes + 64);
    std::memcpy(blob.data(), p.afrag.data(), p.afrag.size() * 2);
    std::memcpy(blob.data() + a_bytes, p.bias0.data(), 16);
    std::memcpy(blob.data() + a_bytes + 16, p.w1.data(), 16);
    if (int st = h->d_mlpx.reserve(blob.size())) return st;
    SYLDET_HIP(hipMemcpy(h->d_mlpx.ptr, blob.data(), blob.size(), hipMemcpyHostToDevice));
    unsigned char *base = (unsigned char *)h->d_mlpx.ptr;
    p.desc.afrag = (const uint4 *)base;
    p.desc.bias0 = (const float *)(base + a_bytes);
    p.desc.w1 = (const float *)(base + a_bytes + 16);
    p.desc.thresholds = (const double *)h->d_thr.ptr;
    return SYLDET_OK;
}

int upload_bdft(syldet *h)
{
    BdftPlan &p = h->bdft;
    auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t b_bytes = pad(p.basis.size() * 2), c_bytes = pad(p.cre.size() * 4), a_bytes = pad(p.afrag.size() * 2);
    std::vector<unsigned char> blob(b_bytes + c_bytes + a_bytes);
    std::memcpy(blob.data(), p.basis.data(), p.basis.size() * 2);
    std::memcpy(blob.data() + b_bytes, p.cre.data(), p.cre.size() * 4);
    std::memcpy(blob.data() + b_bytes + c_bytes, p.afrag.data(), p.afrag.size() * 2);
    if (int st = h->d_bdft.reserve(blob.size())) return st;
    SYLDET_HIP(hipMemcpy(h->d_bdft.ptr, blob.data(), blob.size(), hipMemcpyHostToDevice));
    unsigned char *base = (unsigned char *)h->d_bdft.ptr;
    p.desc.basis = (const uint4 *)base;
    p.desc.cre = (const float *)(base + b_bytes);
    p.desc.afrag = (const uint4 *)(base + b_bytes + c_bytes);
    p.md = h->mlpx.desc;                 // (its device pointers are in place: upload_mlpx ran first)
    p.md.KB = 4;
    p.md.col_stride = 32 * 4 + 8;
    return SYLDET_OK;
}

int build_dft_plan(syldet *h)
{
    if (!plan_dft(h)) return SYLDET_OK;
    if (int st = upload_plan(h, h->dft, h->d_dft)) return st;
    h->dft.desc.spect_power = h->cfg.view.spectrum == SYLDET_SPECTRUM_MAGNITUDE ? 1 : 0;
    h->has_dft = true;
    return SYLDET_OK;
}

// The fold kernel's per-network tables of a multi-network handle: each network's plan, its weight-dependent arrays in one blob per
// network at a fixed stride, then the FusedNet table that points into them.
int upload_fold_nets(syldet *h, const std::vector<std::unique_ptr<OwnedConfig>> &cfgs)
{
    const size_t K = cfgs.size();
    std::vector<FusedPlan> plans(K);
    for (size_t k = 0; k < K; k++) {
        if (!make_fused_plan(cfgs[k]->view, h->geom, plans[k]))
            return fail(SYLDET_ERR_UNSUPPORTED, "fold kernel plan failed for network " + std::to_string(k) + ": " + plans[k].reason);
        // (the shape is shared: compatible networks give the same layout)
        const FusedDesc &a = plans[0].desc, &b = plans[k].desc;
        if (a.s_ok != b.s_ok || a.s2_ok != b.s2_ok || a.s2_nt != b.s2_nt || a.s_padp != b.s_padp || a.s_cs8 != b.s_cs8 ||
            a.s_waves != b.s_waves || a.s_lds_wave != b.s_lds_wave || a.col_shift != b.col_shift || a.H != b.H || a.norm != b.norm)
            return fail(SYLDET_ERR_UNSUPPORTED, "network " + std::to_string(k) + " gives the fold kernel another shape");
    }
    auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    const int n_thr = h->cfg.view.n_thresholds;
    const FusedPlan &p0 = plans[0];
    const size_t sz[10] = {p0.afrag_t.size() * 2, p0.afrag_w.size() * 2, p0.afrag_t2.size() * 2, p0.afrag_w2.size() * 2, p0.bias0.size() * 4,
                           p0.rvec.size() * 4, p0.w1.size() * 4, p0.b1.size() * 4, p0.out_params.size() * 4, (size_t)n_thr * 8};
    size_t off[10], stride = 0;
    for (int i = 0; i < 10; i++) {
        off[i] = stride;
        stride += pad(std::max<size_t>(sz[i], 16));
    }
    std::vector<unsigned char> blob(stride * K + pad(K * sizeof(FusedNet)), 0);
    for (size_t k = 0; k < K; k++) {
        const FusedPlan &p = plans[k];
        const void *src[10] = {p.afrag_t.data(), p.afrag_w.data(), p.afrag_t2.data(), p.afrag_w2.data(), p.bias0.data(),
                               p.rvec.data(), p.w1.data(), p.b1.data(), p.out_params.data(), cfgs[k]->view.thresholds};
        const size_t szk[10] = {p.afrag_t.size() * 2, p.afrag_w.size() * 2, p.afrag_t2.size() * 2, p.afrag_w2.size() * 2, p.bias0.size() * 4,
                                p.rvec.size() * 4, p.w1.size() * 4, p.b1.size() * 4, p.out_params.size() * 4, (size_t)n_thr * 8};
        for (int i = 0; i < 10; i++) {
            if (szk[i] != sz[i]) return fail(SYLDET_ERR_UNSUPPORTED, "network " + std::to_string(k) + " gives the fold kernel tables of another size");
            if (sz[i]) std::memcpy(blob.data() + k * stride + off[i], src[i], sz[i]);
        }
    }
    if (int st = h->d_fnets.reserve(blob.size())) return st;
    const unsigned char *base = (const unsigned char *)h->d_fnets.ptr;
    FusedNet *tab = reinterpret_cast<FusedNet *>(blob.data() + stride * K);
    for (size_t k = 0; k < K; k++) {
        const unsigned char *nb = base + k * stride;
        const FusedDesc &d = plans[k].desc;
        FusedNet &t = tab[k];
        t.afrag_t = (const uint4 *)(nb + off[0]);
        t.afrag_w = (const uint4 *)(nb + off[1]);
        t.afrag_t2 = (const uint4 *)(nb + off[2]);
        t.afrag_w2 = (const uint4 *)(nb + off[3]);
        t.bias0 = (const float *)(nb + off[4]);
        t.rvec = (const float *)(nb + off[5]);
        t.w1 = (const float *)(nb + off[6]);
        t.b1 = (const float *)(nb + off[7]);
        t.out_params = (const float *)(nb + off[8]);
        t.thresholds = (const double *)(nb + off[9]);
        t.w_unscale = d.w_unscale;
        t.guard_r = d.guard_r;
        t.guard_rel_r = d.guard_rel_r;
        t.guard_range_r = d.guard_range_r;
        t.guard_loud = d.guard_loud;
        t.guard_se_abs_r = d.guard_se_abs_r;
    }
    SYLDET_HIP(hipMemcpy(h->d_fnets.ptr, blob.data(), blob.size(), hipMemcpyHostToDevice));
    h->fnets = (const FusedNet *)(base + stride * K);
    return SYLDET_OK;
}

// The generic engine's per-network parameter blobs and thresholds (the network stage and the exact recomputation read them).
int upload_generic_nets(syldet *h, const std::vector<std::unique_ptr<OwnedConfig>> &cfgs)
{
    std::vector<float> all, blob;
    std::vector<double> thr;
    size_t stride = 0;
    for (size_t k = 0; k < cfgs.size(); k++) {
        NetDesc n;
        if (int st = make_net_blob(cfgs[k]->view, h->geom, n, blob)) return st;
        if (k == 0) stride = std::max<size_t>(blob.size(), 1);
        if (blob.size() > stride) return fail(SYLDET_ERR_UNSUPPORTED, "network " + std::to_string(k) + " has a parameter blob of another size");
        blob.resize(stride, 0.0f);
        all.insert(all.end(), blob.begin(), blob.end());
        thr.insert(thr.end(), cfgs[k]->view.thresholds, cfgs[k]->view.thresholds + cfgs[k]->view.n_thresholds);
    }
    if (stride > 0x7fffffff / cfgs.size()) return fail(SYLDET_ERR_UNSUPPORTED, "networks too large for one handle");
    if (int st = h->d_params.reserve(all.size() * sizeof(float))) return st;
    if (int st = h->d_thr.reserve(thr.size() * sizeof(double))) return st;
    SYLDET_HIP(hipMemcpy(h->d_params.ptr, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice));
    SYLDET_HIP(hipMemcpy(h->d_thr.ptr, thr.data(), thr.size() * sizeof(double), hipMemcpyHostToDevice));
    h->net.params = (const float *)h->d_params.ptr;
    h->net.thresholds = (const double *)h->d_thr.ptr;
    h->net.params_stride = (int)stride;
    h->net.thr_stride = h->cfg.view.n_thresholds;
    return SYLDET_OK;
}
}  // namespace

namespace sd {

// A plan for the DFT front half alone: the real STFT geometry with a one-frame, one-unit stand-in network (the
// spectrogram instantiation never touches the network tables).
// (the host half: the plan itself, and whether a fused kernel has a spectrogram instantiation for it)
bool plan_dft(syldet *h)
{
    const syldet_config_t &c = h->cfg.view;
    syldet_config_t sc = c;
    const int F = h->geom.bins;
    // (two layers, F -> 1 -> 1: the class the symmetric-fold kernel's plan is made for)
    std::vector<float> w((size_t)F, 0.0f), b(1, 0.0f), w2(1, 1.0f);
    syldet_layer_t layers[2] = {};
    layers[0].inputs = F; layers[0].outputs = 1; layers[0].transfer = SYLDET_TF_PURELIN; layers[0].weights = w.data(); layers[0].biases = b.data();
    layers[1].inputs = 1; layers[1].outputs = 1; layers[1].transfer = SYLDET_TF_PURELIN; layers[1].weights = w2.data(); layers[1].biases = b.data();
    double thr = 0.0;
    sc.time_range = 1; sc.scaling = SYLDET_SCALING_LINEAR; sc.spectrum = SYLDET_SPECTRUM_POWER;
    sc.n_input_fns = 0; sc.input_fns = nullptr; sc.n_output_fns = 0; sc.output_fns = nullptr;
    sc.n_layers = 2; sc.layers = layers; sc.n_thresholds = 1; sc.thresholds = &thr;
    syldet_geometry_t sg = h->geom;
    sg.inputs = F; sg.outputs = 1;
    if (!make_fused_plan(sc, sg, h->dft)) return false;              // not applicable: the generic FFT stays
    // (two spectrogram instantiations: the fold kernel's twice-folded form for 256-point frames under a 256-sample window,
    // the 8-wave kernel's for its shapes)
    return h->dft.desc.classic_ok || fused_s_spectrogram_applicable(h->dft.desc);
}

// Does the network's input chain start with a scale-invariant normaliser (l2normalize, normalize, normalizestd:
// NeuralNet.swift:41-109)?  Behind one, the network sees a unit-scale vector whatever the recording's level, and the
// matrix-core transforms' error -- 2^-21.4 of a frame's column level -- is 2^-21.4 of that unit.  Without one the network sees
// the columns at the recording's level, and the same relative error grows with it where an fp32 FFT's is eight times smaller:
// AUTO then keeps true fp32 transforms, except on the fold kernel, which knows when the level makes the difference and
// recomputes those evaluations exactly (guard_loud, fused_plan.cpp).
bool normalised_chain(const syldet_config_t &c)
{
    return c.n_input_fns > 0 && (c.input_fns[0].kind == SYLDET_FN_L2NORMALIZE || c.input_fns[0].kind == SYLDET_FN_NORMALIZE ||
                                 c.input_fns[0].kind == SYLDET_FN_NORMALIZESTD);
}

int64_t count_frames(const syldet *h, int64_t S) { return count_frames(h->geom, h->cfg.view.window_length, S); }
int64_t count_evals(const syldet *h, int64_t S) { return count_evals(h->geom, h->cfg.view.window_length, h->cfg.view.time_range, S); }

// Would a handle of this one network, created under AUTO, run its batches on the fold kernel (syldet_create's rule plus the
// launcher's choice, the SYLDET_* switches included)?  `fused_ok`: the fold kernel takes the shape at all (SYLDET_ENGINE_FUSED).
bool takes_fold(const syldet_config_t &c, const syldet_geometry_t &g, const syldet::Switches &sw, bool &fused_ok)
{
    fused_ok = false;
    FusedPlan plan;
    if (!make_fused_plan(c, g, plan) || !fused_s_applicable(plan.desc)) return false;
    FusedDesc d = plan.desc;
    apply_switches(sw, d);
    fused_ok = fused_choice(d, 1) == 2;
    // AUTO: log / dB columns only behind l2normalize; linear ones on any chain the fold kernel takes
    return fused_ok && (c.scaling == SYLDET_SCALING_LINEAR || d.norm == 1);
}

// A multi-network handle's networks: owned copies, every one compatible with network 0, and whether all of them would run on
// the fold kernel under AUTO (`fold`) / take it at all (`fused_ok`) -- host work only.
int survey_nets(const syldet_config_t *const *cfgs, int32_t n_nets, std::vector<std::unique_ptr<OwnedConfig>> &own, bool &fold, bool &fused_ok)
{
    syldet::Switches sw;
    sw.read();
    fold = fused_ok = true;
    try {
        for (int32_t i = 0; i < n_nets; i++) {
            own.emplace_back(new OwnedConfig());
            if (int st = own.back()->assign(*cfgs[i])) return st;
            syldet_geometry_t g{};
            if (int st = compute_geometry(own.back()->view, &g)) return st;
            const char *field = nullptr;
            const int cmp = syldet_config_compatible(cfgs[0], cfgs[i], &field);
            if (cmp < 0) return cmp;
            if (cmp == 0)
                return fail(SYLDET_ERR_UNSUPPORTED, "network " + std::to_string(i) + " is not compatible with network 0: " + field +
                                                        " differs (networks that differ there need a handle each)");
            bool ok = false;
            if (!takes_fold(own.back()->view, g, sw, ok)) fold = false;
            if (!ok) fused_ok = false;
        }
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    return SYLDET_OK;
}

// syldet_create's choice between the fused and the generic engine for a handle whose configuration, geometry and switches are in
// place (host work only: the fused plan is made here, uploaded later).
int choose_engine(syldet *h, int engine)
{
    h->engine_asked = engine;
    h->engine = SYLDET_ENGINE_GENERIC;
    if (engine != SYLDET_ENGINE_GENERIC && engine != SYLDET_ENGINE_WIDE_BF16) {
        // The fused engine hands columns to the first layer as f16 hi + lo pairs.  For linear |X| columns that is below
        // fp32 noise; log / dB values (magnitude up to ~100, 2^-22 relative = a few 1e-5 absolute) can leave the 1e-5
        // parity bar.  AUTO therefore keeps those scalings on the generic engine; the fused one stays available on request.
        // Round 3: the symmetric-fold kernel transforms every frame at its own scale -- a bin's error is relative to its frame,
        // as the generic FFT's is -- so behind l2normalize (what the split of the logarithms loses is lost relative to the vector
        // the network sees, as in the generic engine's matrix-core network stage) AUTO takes it for log / dB columns too.
        const bool strict_ok = h->cfg.view.scaling == SYLDET_SCALING_LINEAR;
        if (engine == SYLDET_ENGINE_AUTO && !strict_ok) {
            if (make_fused_plan(h->cfg.view, h->geom, h->fused) && fused_s_applicable(h->fused.desc) && h->fused.desc.norm == 1 &&
                !h->sw.fused_nofold && !h->sw.fused_classic) {
                h->engine = SYLDET_ENGINE_FUSED;
            } else {
                h->fused = FusedPlan();
                h->fused.reason = "log/dB scaling: AUTO keeps the generic engine for 1e-5 parity";
            }
        } else if (make_fused_plan(h->cfg.view, h->geom, h->fused)) {
            const bool fold = fused_s_applicable(h->fused.desc) && !h->sw.fused_nofold && !h->sw.fused_classic;
            if (engine == SYLDET_ENGINE_AUTO && !normalised_chain(h->cfg.view) && !fold) {
                // no normaliser in front of the network: the pass-scaled kernels' error follows the recording's level
                // (normalised_chain above); only the fold kernel guards against that
                h->fused = FusedPlan();
                h->fused.reason = "no normaliser in front of the network: AUTO keeps fp32 transforms outside the fold kernel's class";
            } else {
                h->engine = SYLDET_ENGINE_FUSED;
            }
        } else if (engine == SYLDET_ENGINE_FUSED) {
            return fail(SYLDET_ERR_UNSUPPORTED, "fused engine not available for this configuration: " + h->fused.reason);
        }
    }
    return SYLDET_OK;
}
}  // namespace sd

void sd::bank_info(const syldet_t *h, sd::BankInfo *out)
{
    *out = sd::BankInfo{h->channels, h->device, h->cfg.view.sampling_rate, h->cfg.view.window_length, h->cfg.view.time_range, h->geom,
                        !h->classes.empty() ? h->bank_net.data() : h->net_of.empty() ? nullptr : h->net_of.data()};
}

extern "C" {

int syldet_create(const syldet_config_t *cfg, int32_t n_channels, int32_t device, int32_t engine, syldet_t **out)
{
    if (!cfg || !out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (n_channels <= 0 || n_channels > 65535)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_channels must be in [1, 65535]");
    if (!engine_known(engine)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "unknown engine");
    std::unique_ptr<syldet> h(new (std::nothrow) syldet());
    if (!h) return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    if (int st = h->cfg.assign(*cfg)) return st;
    if (int st = compute_geometry(h->cfg.view, &h->geom)) return st;
    h->sw.read();
    if (h->sw.host_chunk > 0) h->host_chunk_bytes = (size_t)h->sw.host_chunk;

    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0)
        return fail(SYLDET_ERR_NO_DEVICE, std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count is 0"));
    if (device < 0 || device >= n_dev) return fail(SYLDET_ERR_NO_DEVICE, "device index out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(SYLDET_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SYLDET_ERR_NO_DEVICE, std::string("libsyldet is built for gfx950 only, found ") + prop.gcnArchName);
    SYLDET_HIP(hipSetDevice(device));
    h->device = device;
    h->channels = n_channels;
    if (int st = choose_engine(h.get(), engine)) return st;
    h->geom.engine = h->engine;
    SYLDET_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    // (from here on a failure takes the stream and the tables with it: syldet_destroy, not delete)
    struct Undo { std::unique_ptr<syldet> &h; ~Undo() { if (h) syldet_destroy(h.release()); } } undo{h};
    if (int st = build_tables(h.get())) return st;
    if (h->engine == SYLDET_ENGINE_FUSED) {
        if (int st = upload_fused(h.get())) return st;
        if (int st = upload_fix(h.get())) return st;
    }
    // AUTO on the generic engine: the network stage goes to the matrix cores where the configuration is of that kernel's
    // class (a handle created for SYLDET_ENGINE_GENERIC keeps the reference's operation order throughout)
    if (engine == SYLDET_ENGINE_AUTO && h->engine == SYLDET_ENGINE_GENERIC && !h->sw.no_mlpx && make_mlpx_plan(h->cfg.view, h->geom, h->mlpx)) {
        if (int st = upload_mlpx(h.get())) return st;
        if (make_bdft_plan(h->cfg.view, h->geom, h->mlpx, h->bdft))
            if (int st = upload_bdft(h.get())) return st;
    }
    if (engine != SYLDET_ENGINE_GENERIC) {
        if (int st = build_dft_plan(h.get())) return st;
        if (h->has_dft && !h->has_fix)
            if (int st = upload_fix(h.get())) return st;
    }
    if (engine == SYLDET_ENGINE_WIDE_BF16) {
        std::string why;
        if (int st = upload_wide(h.get(), why)) return why.empty() ? st : fail(st, "wide-network engine not available for this configuration: " + why);
        h->engine = SYLDET_ENGINE_WIDE_BF16;
        h->geom.engine = h->engine;
    }
    // the reference's sample ring (409 600 bytes) + what its feature ring would still hold as columns
    uint64_t need = (uint64_t)(kSampleRingBytes / 4) + (uint64_t)h->geom.gap + (uint64_t)h->cfg.view.window_length +
                    (uint64_t)(h->cfg.view.time_range + 1) * (uint64_t)h->geom.hop, cap = 1;
    while (cap < need) cap <<= 1;
    try {
        h->streams.resize((size_t)n_channels);
        for (auto &s : h->streams) {
            s.reset(new ChannelStream());
            s->last.assign((size_t)h->geom.outputs, 0.0f);   // lastOutputs zeros, SyllableDetector.swift:70
            s->mask = cap - 1;
        }
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    *out = h.release();
    return SYLDET_OK;
}

int syldet_config_compatible(const syldet_config_t *a, const syldet_config_t *b, const char **field)
{
    if (field) *field = nullptr;
    if (!a || !b) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    for (const syldet_config_t *x : {a, b})
        if ((x->n_input_fns > 0 && !x->input_fns) || (x->n_output_fns > 0 && !x->output_fns) || (x->n_layers > 0 && !x->layers))
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL array in a configuration");
    syldet_geometry_t ga{}, gb{};
    if (int st = compute_geometry(*a, &ga)) return st;
    if (int st = compute_geometry(*b, &gb)) return st;
    // the first difference in the framing or the shape of the chain: its name (a static string) and, in the last error, where
    auto differ = [field](const char *name, int index) {
        if (field) *field = name;
        set_error(index < 0 ? std::string("configurations differ in ") + name
                            : std::string("configurations differ in ") + name + " (entry " + std::to_string(index) + ")");
        return 0;
    };
    if (a->sampling_rate != b->sampling_rate) return differ("sampling_rate", -1);
    if (a->fourier_length != b->fourier_length) return differ("fourier_length", -1);
    if (a->window_length != b->window_length) return differ("window_length", -1);
    if (a->window_overlap != b->window_overlap) return differ("window_overlap", -1);
    if (a->time_range != b->time_range) return differ("time_range", -1);
    if (ga.f0 != gb.f0 || ga.f1 != gb.f1) return differ("band", -1);          // freq_lo / freq_hi may differ, the bins they give may not
    if (a->scaling != b->scaling) return differ("scaling", -1);
    if (a->window != b->window) return differ("window", -1);
    if (a->spectrum != b->spectrum) return differ("spectrum", -1);
    if (a->rule != b->rule) return differ("rule", -1);
    if (a->n_input_fns != b->n_input_fns) return differ("n_input_fns", -1);
    for (int i = 0; i < a->n_input_fns; i++) {
        if (a->input_fns[i].kind != b->input_fns[i].kind) return differ("input_fns.kind", i);
    }
    if (a->n_output_fns != b->n_output_fns) return differ("n_output_fns", -1);
    for (int i = 0; i < a->n_output_fns; i++) {
        if (a->output_fns[i].kind != b->output_fns[i].kind) return differ("output_fns.kind", i);
    }
    if (a->n_layers != b->n_layers) return differ("n_layers", -1);
    for (int l = 0; l < a->n_layers; l++) {
        if (a->layers[l].inputs != b->layers[l].inputs) return differ("layers.inputs", l);
        if (a->layers[l].outputs != b->layers[l].outputs) return differ("layers.outputs", l);
        if (a->layers[l].transfer != b->layers[l].transfer) return differ("layers.transfer", l);
    }
    if (a->n_thresholds != b->n_thresholds) return differ("n_thresholds", -1);
    // (the functions' vector lengths follow from the layers: a valid configuration's maps have inputs / outputs entries)
    return 1;
}

// syldet_create_multi, and (mixed_class) the handle of one class of a mixed bank: the same engine choice and the same kernels,
// but one network makes no plain handle there -- on the fold kernel it takes the multi-network form (the form with the row
// table), and elsewhere the generic engine as SYLDET_ENGINE_GENERIC has it (the engines without a multi-network form have no
// row table either).
static int create_multi_impl(const syldet_config_t *const *cfgs, int32_t n_nets, const int32_t *channel_net, int32_t n_channels,
                             int32_t device, int32_t engine, syldet_t **out, bool mixed_class)
{
    if (!cfgs || !channel_net || !out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (n_nets < 1) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_nets must be >= 1");
    if (n_channels <= 0 || n_channels > 65535) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_channels must be in [1, 65535]");
    if (!engine_known(engine)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "unknown engine");
    for (int32_t i = 0; i < n_nets; i++)
        if (!cfgs[i]) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL configuration " + std::to_string(i));
    for (int32_t c = 0; c < n_channels; c++)
        if (channel_net[c] < 0 || channel_net[c] >= n_nets)
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "channel_net[" + std::to_string(c) + "] = " + std::to_string(channel_net[c]) + " is outside [0, n_nets)");
    if (engine == SYLDET_ENGINE_WIDE_BF16) return fail(SYLDET_ERR_UNSUPPORTED, "the wide-network engine has no multi-network form");
    std::vector<std::unique_ptr<OwnedConfig>> own;
    bool fold = true, fused_ok = true;
    if (int st = survey_nets(cfgs, n_nets, own, fold, fused_ok)) return st;
    // one network: exactly a syldet_create handle
    if (n_nets == 1 && !mixed_class) return syldet_create(cfgs[0], n_channels, device, engine, out);
    if (engine == SYLDET_ENGINE_FUSED && !fused_ok)
        return fail(SYLDET_ERR_UNSUPPORTED, "fused engine on a multi-network handle: only the fold kernel has that form, and it does not take this shape");
    const bool on_fold = engine == SYLDET_ENGINE_FUSED || (engine == SYLDET_ENGINE_AUTO && fold);
    if (n_nets == 1 && !on_fold) return syldet_create(cfgs[0], n_channels, device, SYLDET_ENGINE_GENERIC, out);
    // network 0 makes the handle -- the device, the shape's tables, the streams -- on the fold kernel or on the generic engine
    // exactly as SYLDET_ENGINE_GENERIC has it; the other networks' tables follow
    syldet_t *raw = nullptr;
    if (int st = syldet_create(cfgs[0], n_channels, device, on_fold ? engine : SYLDET_ENGINE_GENERIC, &raw)) return st;
    std::unique_ptr<syldet, int (*)(syldet_t *)> h(raw, syldet_destroy);
    if (on_fold && h->engine != SYLDET_ENGINE_FUSED) return fail(SYLDET_ERR_UNSUPPORTED, "the fold kernel did not take network 0");
    try {
        if (n_nets == 1) {                                        // (a mixed bank's one-network class on the fold kernel)
            if (int st = h->d_net_of.reserve((size_t)n_channels * sizeof(int))) return st;
            SYLDET_HIP(hipMemset(h->d_net_of.ptr, 0, (size_t)n_channels * sizeof(int)));
            if (int st = upload_fold_nets(h.get(), own)) return st;
            *out = h.release();
            return SYLDET_OK;
        }
        h->n_nets = n_nets;
        h->net_of.assign(channel_net, channel_net + n_channels);
        for (int32_t c = 0; c < n_channels; c++) {
            const syldet_config_t &v = own[(size_t)channel_net[c]]->view;
            h->chan_thr0.push_back(v.thresholds[0]);
            h->chan_thr.insert(h->chan_thr.end(), v.thresholds, v.thresholds + v.n_thresholds);
        }
        if (int st = h->d_net_of.reserve((size_t)n_channels * sizeof(int))) return st;
        SYLDET_HIP(hipMemcpy(h->d_net_of.ptr, h->net_of.data(), (size_t)n_channels * sizeof(int), hipMemcpyHostToDevice));
        if (int st = upload_generic_nets(h.get(), own)) return st;
        h->fused.desc.thresholds = h->net.thresholds;            // (network 0's, first in the table that replaced its own)
        if (on_fold)
            if (int st = upload_fold_nets(h.get(), own)) return st;
        h->net_cfgs = std::move(own);
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    *out = h.release();
    return SYLDET_OK;
}

int syldet_create_multi(const syldet_config_t *const *cfgs, int32_t n_nets, const int32_t *channel_net, int32_t n_channels,
                        int32_t device, int32_t engine, syldet_t **out)
{
    return create_multi_impl(cfgs, n_nets, channel_net, n_channels, device, engine, out, false);
}

int syldet_config_same_clock(const syldet_config_t *a, const syldet_config_t *b, const char **field)
{
    if (field) *field = nullptr;
    if (!a || !b) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    for (const syldet_config_t *x : {a, b})
        if ((x->n_input_fns > 0 && !x->input_fns) || (x->n_output_fns > 0 && !x->output_fns) || (x->n_layers > 0 && !x->layers))
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL array in a configuration");
    syldet_geometry_t ga{}, gb{};
    if (int st = compute_geometry(*a, &ga)) return st;
    if (int st = compute_geometry(*b, &gb)) return st;
    auto differ = [field](const char *name) {
        if (field) *field = name;
        set_error(std::string("configurations differ in ") + name + " (the evaluation clock)");
        return 0;
    };
    // (these fix gap, hop, first_index, the evaluation count and the [C][E][n_out] layout; valid configurations have
    // n_thresholds == the last layer's outputs)
    if (a->sampling_rate != b->sampling_rate) return differ("sampling_rate");
    if (a->window_length != b->window_length) return differ("window_length");
    if (a->window_overlap != b->window_overlap) return differ("window_overlap");
    if (a->time_range != b->time_range) return differ("time_range");
    if (a->n_thresholds != b->n_thresholds || ga.outputs != gb.outputs) return differ("n_thresholds");
    return 1;
}

int syldet_create_mixed(const syldet_config_t *const *cfgs, int32_t n_nets, const int32_t *channel_net, int32_t n_channels,
                        int32_t device, int32_t engine, syldet_t **out)
{
    if (!cfgs || !channel_net || !out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (n_nets < 1) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_nets must be >= 1");
    if (n_channels <= 0 || n_channels > 65535) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_channels must be in [1, 65535]");
    if (!engine_known(engine)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "unknown engine");
    for (int32_t i = 0; i < n_nets; i++)
        if (!cfgs[i]) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL configuration " + std::to_string(i));
    for (int32_t c = 0; c < n_channels; c++)
        if (channel_net[c] < 0 || channel_net[c] >= n_nets)
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "channel_net[" + std::to_string(c) + "] = " + std::to_string(channel_net[c]) + " is outside [0, n_nets)");
    // every network valid on its own (syldet_create's statuses) and on network 0's clock
    std::vector<int> cls((size_t)n_nets, -1), rep;          // a network's class; each class's first network
    syldet::Switches sw;
    sw.read();
    try {
        for (int32_t i = 0; i < n_nets; i++) {
            OwnedConfig own;
            if (int st = own.assign(*cfgs[i])) return st;
            syldet_geometry_t g{};
            if (int st = compute_geometry(own.view, &g)) return st;
            const char *field = nullptr;
            const int cmp = syldet_config_same_clock(cfgs[0], cfgs[i], &field);
            if (cmp < 0) return cmp;
            if (cmp == 0)
                return fail(SYLDET_ERR_UNSUPPORTED, "network " + std::to_string(i) + " does not share network 0's evaluation clock: " + field +
                                                        " differs (networks that differ there need a handle each)");
            // the classes: syldet_config_compatible is field equality, so comparing with each class's first network partitions
            for (size_t k = 0; k < rep.size() && cls[(size_t)i] < 0; k++)
                if (syldet_config_compatible(cfgs[rep[k]], cfgs[i], nullptr) == 1) cls[(size_t)i] = (int)k;
            if (cls[(size_t)i] < 0) {
                cls[(size_t)i] = (int)rep.size();
                rep.push_back(i);
            }
        }
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    if (engine == SYLDET_ENGINE_WIDE_BF16) return fail(SYLDET_ERR_UNSUPPORTED, "the wide-network engine has no mixed-bank form");
    // all compatible (one network included): exactly a syldet_create_multi handle
    if (rep.size() == 1) return syldet_create_multi(cfgs, n_nets, channel_net, n_channels, device, engine, out);
    // each class that has channels: its networks (in file order), the class-local network of each of its channels, its rows
    struct Class { std::vector<int32_t> nets, local_net, rows; };
    std::vector<Class> classes;
    std::vector<int> slot(rep.size(), -1);                  // class -> index in `classes` (classes without channels are left out)
    std::vector<int> class_of((size_t)n_channels), local_of((size_t)n_channels);
    try {
        for (int32_t c = 0; c < n_channels; c++) {
            const int k = cls[(size_t)channel_net[c]];
            if (slot[(size_t)k] < 0) {
                slot[(size_t)k] = (int)classes.size();
                classes.emplace_back();
                for (int32_t i = 0; i < n_nets; i++)
                    if (cls[(size_t)i] == k) classes.back().nets.push_back(i);
            }
            Class &cl = classes[(size_t)slot[(size_t)k]];
            const int32_t ln = (int32_t)(std::find(cl.nets.begin(), cl.nets.end(), channel_net[c]) - cl.nets.begin());
            class_of[(size_t)c] = slot[(size_t)k];
            local_of[(size_t)c] = (int)cl.rows.size();
            cl.local_net.push_back(ln);
            cl.rows.push_back(c);
        }
        // FUSED: every class on the fold kernel, or nothing (refused before any device is touched)
        if (engine == SYLDET_ENGINE_FUSED)
            for (const Class &cl : classes)
                for (int32_t i : cl.nets) {
                    OwnedConfig own;
                    if (int st = own.assign(*cfgs[i])) return st;
                    syldet_geometry_t g{};
                    if (int st = compute_geometry(own.view, &g)) return st;
                    bool ok = false;
                    (void)takes_fold(own.view, g, sw, ok);
                    if (!ok)
                        return fail(SYLDET_ERR_UNSUPPORTED, "fused engine on a mixed bank: network " + std::to_string(i) +
                                                                "'s class does not take the fold kernel (the only fused kernel with a row table)");
                }
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    // the bank: the clock, the channels' streaming state, the stream (the first class's first network on the generic engine;
    // its own tables are never launched)
    syldet_t *raw = nullptr;
    if (int st = syldet_create(cfgs[classes[0].nets[0]], n_channels, device, SYLDET_ENGINE_GENERIC, &raw)) return st;
    std::unique_ptr<syldet, int (*)(syldet_t *)> h(raw, syldet_destroy);
    try {
        for (const Class &cl : classes) {
            std::vector<const syldet_config_t *> cc;
            for (int32_t i : cl.nets) cc.push_back(cfgs[i]);
            syldet_t *kr = nullptr;
            if (int st = create_multi_impl(cc.data(), (int32_t)cc.size(), cl.local_net.data(), (int32_t)cl.rows.size(), device, engine, &kr, true))
                return st;
            std::unique_ptr<syldet, int (*)(syldet_t *)> k(kr, syldet_destroy);
            // (the classes launch on the bank's stream: no stream of their own)
            if (k->stream) {
                SYLDET_HIP(hipStreamDestroy(k->stream));
                k->stream = nullptr;
            }
            k->root = h.get();
            k->rows.assign(cl.rows.begin(), cl.rows.end());
            if (int st = k->d_row_of.reserve(k->rows.size() * sizeof(int))) return st;
            SYLDET_HIP(hipMemcpy(k->d_row_of.ptr, k->rows.data(), k->rows.size() * sizeof(int), hipMemcpyHostToDevice));
            h->classes.push_back(std::move(k));
        }
        h->class_of = std::move(class_of);
        h->local_of = std::move(local_of);
        h->bank_net.assign(channel_net, channel_net + n_channels);
        for (int32_t c = 0; c < n_channels; c++) {
            const syldet_config_t *v = cfgs[channel_net[c]];
            h->chan_thr0.push_back(v->thresholds[0]);
            h->chan_thr.insert(h->chan_thr.end(), v->thresholds, v->thresholds + v->n_thresholds);
        }
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    // what differs between the classes is -1 in the bank's geometry (syldet_channel_geometry has each channel's own)
    syldet_geometry_t &g = h->geom;
    g = h->classes[0]->geom;
    for (const auto &k : h->classes) {
        const syldet_geometry_t &o = k->geom;
        if (o.f0 != g.f0) g.f0 = -1;
        if (o.f1 != g.f1) g.f1 = -1;
        if (o.bins != g.bins) g.bins = -1;
        if (o.inputs != g.inputs) g.inputs = -1;
        if (o.engine != g.engine) g.engine = -1;
    }
    *out = h.release();
    return SYLDET_OK;
}

int syldet_channel_geometry(const syldet_t *h, int32_t channel, syldet_geometry_t *out)
{
    if (!h || !out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (channel < 0 || channel >= h->channels) return fail(SYLDET_ERR_INVALID_ARGUMENT, "channel outside the bank");
    *out = h->classes.empty() ? h->geom : h->classes[(size_t)h->class_of[(size_t)channel]]->geom;
    return SYLDET_OK;
}

int syldet_destroy(syldet_t *h)
{
    if (!h) return SYLDET_OK;
    forget_call(h);
    (void)hipSetDevice(h->device);
    if (h->stream) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipStreamDestroy(h->stream);
    }
    for (hipEvent_t e : h->events)
        if (e) (void)hipEventDestroy(e);
    if (h->prof_items) (void)hipHostFree(h->prof_items);
    for (DeviceBuffer *b : {&h->d_window, &h->d_tw, &h->d_sw, &h->d_params, &h->d_thr, &h->d_columns, &h->d_fused, &h->d_mlpx, &h->d_bdft, &h->d_stamps, &h->d_fix,
                            &h->d_ctab, &h->d_planar, &h->d_widen, &h->d_wide, &h->d_xn, &h->d_dft, &h->d_net_of, &h->d_fnets, &h->d_row_of, &h->d_stage_net, &h->d_stage_in,
                            &h->d_stage_out, &h->d_stage_flags, &h->d_stage_idx, &h->d_stage_cnt, &h->d_trace, &h->d_trigger_last, &h->d_trigger, &h->d_levels_part,
                            &h->d_levels})
        b->release();
    for (DeviceBuffer &b : h->d_trace_thr) b.release();
    h->p_stage_in.release();
    h->p_stage_out.release();
    for (int b = 0; b < 2; b++) {
        h->pipe.d_in[b].release(); h->pipe.d_out[b].release(); h->pipe.d_fl[b].release();
        for (hipEvent_t e : {h->pipe.ev_h2d[b], h->pipe.ev_k[b], h->pipe.ev_d2h[b]})
            if (e) (void)hipEventDestroy(e);
    }
    if (h->pipe.s_in) (void)hipStreamDestroy(h->pipe.s_in);
    if (h->pipe.s_out) (void)hipStreamDestroy(h->pipe.s_out);
    delete h;
    return SYLDET_OK;
}

int syldet_get_geometry(const syldet_t *h, syldet_geometry_t *out)
{
    if (!h || !out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = h->geom;
    return SYLDET_OK;
}

int32_t syldet_channels(const syldet_t *h) { return h ? h->channels : 0; }

int syldet_profile(syldet_t *h, int enable)
{
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    h->profiling = enable != 0;
    h->prof_seq = 0;
    h->prof_calls.clear();
    return SYLDET_OK;
}

int syldet_profile_history(syldet_t *h, int32_t calls)
{
    if (!h || calls < 1 || calls > 65536) return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (hipEvent_t e : h->events)
        if (e) (void)hipEventDestroy(e);
    h->events.clear();
    h->prof_calls.clear();
    h->prof_depth = calls;
    h->prof_seq = 0;
    return SYLDET_OK;
}

int syldet_timings(syldet_t *h, int32_t calls_back, double *milliseconds, const char **names, int32_t capacity, int32_t *count)
{
    if (!h || !count || capacity < 0 || (capacity > 0 && !milliseconds) || calls_back < 0)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    *count = 0;
    if (h->prof_calls.empty() || calls_back >= h->prof_depth || (int64_t)calls_back >= h->prof_seq) return SYLDET_OK;
    const int idx = (int)((h->prof_seq - 1 - calls_back) % h->prof_depth);
    const syldet::ProfCall &pc = h->prof_calls[(size_t)idx];
    int n = 0;
    for (int i = 0; i < pc.count; i++) {
        const size_t base = (size_t)(idx * syldet::kMaxTimed + i) * 2;
        SYLDET_HIP(hipEventSynchronize(h->events[base + 1]));
        if (n < capacity) {
            float ms = 0.0f;
            SYLDET_HIP(hipEventElapsedTime(&ms, h->events[base], h->events[base + 1]));
            milliseconds[n] = (double)ms;
            if (names) names[n] = pc.names[i];
        }
        n++;
    }
    // the exact path, behind the call's kernels: listed for calls that gave it work, with the duration it measured itself (timed_fixup)
    if (pc.fix && h->prof_items && idx < h->prof_items_n) {
        if (hipStreamSynchronize(pc.fix_stream) != hipSuccess) {       // (a caller's stream that is gone by now: everything, then)
            (void)hipGetLastError();
            SYLDET_HIP(hipDeviceSynchronize());
        }
        if (h->prof_items[2 * idx] != 0u) {
            if (n < capacity) {
                milliseconds[n] = (double)h->prof_items[2 * idx + 1] * 1e-5;
                if (names) names[n] = kFixupName;
            }
            n++;
        }
    }
    *count = n;
    return SYLDET_OK;
}

int syldet_last_timings(syldet_t *h, double *milliseconds, const char **names, int32_t capacity, int32_t *count)
{
    return syldet_timings(h, 0, milliseconds, names, capacity, count);
}

int syldet_fixup_stats(syldet_t *h, int64_t *items, int32_t *overflow)
{
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    int64_t n = 0;
    int32_t of = 0;
    // (a mixed bank: its classes' lists, summed)
    std::vector<syldet *> hs;
    if (h->classes.empty()) hs.push_back(h);
    for (auto &k : h->classes) hs.push_back(k.get());
    for (syldet *x : hs) {
        unsigned c[4] = {0, 0, 0, 0};
        if (x->d_fix.ptr) {
            SYLDET_HIP(hipSetDevice(x->device));
            SYLDET_HIP(hipMemcpy(c, x->d_fix.ptr, sizeof(c), hipMemcpyDeviceToHost));
        }
        n += (int64_t)c[2];
        of |= (int32_t)c[3];
    }
    if (items) *items = n;
    if (overflow) *overflow = of;
    return SYLDET_OK;
}

int64_t syldet_count_frames(const syldet_t *h, int64_t n_samples) { return h ? count_frames(h, n_samples) : -1; }
int64_t syldet_count_evals(const syldet_t *h, int64_t n_samples) { return h ? count_evals(h, n_samples) : -1; }

// Host memory for audio and results that the device reads and writes in place (page-locked): what the reference's ring
// allocation (TPCircularBufferInit, TPCircularBuffer.c:43-124: the buffer the audio thread produces into) becomes for a
// host that feeds a GPU.  Buffers from here make syldet_run skip its staging copies.
int syldet_host_alloc(size_t bytes, void **out)
{
    if (!out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes > 0 ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) {
        *out = nullptr;
        return fail(e == hipErrorOutOfMemory ? SYLDET_ERR_OUT_OF_MEMORY : SYLDET_ERR_DEVICE, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    }
    return SYLDET_OK;
}

int syldet_host_free(void *p)
{
    if (!p) return SYLDET_OK;
    SYLDET_HIP(hipHostFree(p));
    return SYLDET_OK;
}

}  // extern "C"
