// syldet_train.cpp -- training (include/syldet.h, "training"; kernels_train.hip): the trainer that keeps a packed plan's detectors,
// the caller's labels, the network's fixed part and the partial sums on the device, so that syldet_train_targets_device with the
// same labels and every syldet_train_gradient_device are launches only; and the targets on the host (train_targets.hpp, one detector).
// Training from the tool (include/syldet.h): the input range of the chain in front of the first mapminmax and the trainer's own
// copy of that map, the Adam step on the moments the trainer keeps, and the fit that enqueues gradient, combine and step.
// Training a network per channel (syldet_trainer_create_multi): the same trainer with N networks' fixed parts and the group tables
// (kernels.hpp, TrainMulti) on the device; its calls launch the multi form of the kernels (kernels_train_multi.hip).

#include "syldet_handle.hpp"
#include "train_adam.hpp"
#include "train_targets.hpp"

static_assert(SYLDET_TRAIN_MAX_HIDDEN == sd::kTrainMaxHidden && SYLDET_TRAIN_MAX_OUTPUTS == sd::kTrainMaxOut, "the header's limits are the kernel's");

struct syldet_trainer : sd::DetectorTable {  // (the spans: evaluations)
    int P = 0;
    int64_t row_frames = 0;                  // (packed) what n_frames must be
    sd::TrainDesc desc{};
    sd::DeviceBuffer d_fixed;                // maps [N] | (packed) by_row [D] | row_begin [rows + 1] | (multi) TrainDesc [N] | rows by network | net_row_begin [N + 1]
    sd::DeviceBuffer d_part;                 // [N][max_groups][P + 2] fp64
    sd::DeviceBuffer d_opt;                  // the optimiser's: loss [N][2] fp64 | gradient [N][P] | m [N][P] | v [N][P] fp32
    int map_at = -1;                         // the first mapminmax input function (-1: none) and the host's copy of its parameters
    std::vector<float> map;                  // [N] x_offsets [I] | gains [I]
    // the multi form (syldet_trainer_create_multi; N = 1 and multi = false: the plain trainer, whose launches read desc alone)
    bool multi = false;
    int N = 1;
    int maps_per = 0;                        // floats a network has in maps
    std::vector<int32_t> row_net, net_rows;  // [rows] a row's network; [N] the rows a network has
    std::vector<sd::TrainDesc> descs;        // [N] every network's own (desc is network 0's); on the device at descs_at of d_fixed
    size_t descs_at = 0;
    sd::TrainMulti mu{};
    const sd::DetSpan *d_dets = nullptr;
    const int32_t *d_row_begin = nullptr;
    hipStream_t last = nullptr;              // the stream of the last call that may still read the labels or write the partials
    // the kept labels
    bool has_labels = false, has_output = false;
    std::vector<int64_t> begin, labels;      // [D + 1], [n_labels]
    std::vector<int32_t> output;             // [n_labels]
    sd::DeviceBuffer d_labels;               // label_begin | labels | label_output
};

namespace {

int two_layers(const syldet_config_t &c, int *I, int *H, int *O)
{
    if (c.n_layers != 2 || !c.layers) return fail(SYLDET_ERR_UNSUPPORTED, "the trainer takes networks of exactly two layers");
    if (c.layers[0].inputs < 1 || c.layers[0].outputs < 1 || c.layers[1].outputs < 1 || c.layers[1].inputs != c.layers[0].outputs)
        return fail(SYLDET_ERR_LAYER_SHAPE, "the two layers do not fit each other");
    *I = c.layers[0].inputs;
    *H = c.layers[0].outputs;
    *O = c.layers[1].outputs;
    return SYLDET_OK;
}

int class_weights(float wp, float wn)
{
    if (!(wp >= 0.0f) || !(wn >= 0.0f)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "a class weight is NaN or negative");
    return SYLDET_OK;
}

int half_width_arg(int64_t hw)
{
    if (hw < 0 || hw > sd::kTrainMaxHalfWidth) return fail(SYLDET_ERR_INVALID_ARGUMENT, "half_width_samples must be in [0, 2^40]");
    return SYLDET_OK;
}

int outputs_arg(const int32_t *label_output, int64_t n, int O)
{
    if (label_output)
        for (int64_t j = 0; j < n; j++)
            if (label_output[j] < 0 || label_output[j] >= O)
                return fail(SYLDET_ERR_INVALID_ARGUMENT, "label_output[" + std::to_string(j) + "] = " + std::to_string(label_output[j]) + " is outside [0, " +
                                                             std::to_string(O) + ")");
    return SYLDET_OK;
}

// what the gradient, the range and the fit check of their columns; row_stride 0 becomes a row's elements
int columns_args(const syldet_trainer *t, int64_t n_evals, int64_t n_frames, int64_t *row_stride)
{
    if (n_evals < 0 || n_frames < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_evals or n_frames is negative");
    const sd::TrainDesc &d = t->desc;
    if (t->packed && (n_evals != t->row_units || n_frames != t->row_frames))
        return t->packed_rows_refusal("n_evals and n_frames", std::to_string(t->row_units) + " evaluations and " + std::to_string(t->row_frames) + " frames");
    if (n_evals > 0 && n_frames < n_evals + d.T - 1)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, std::to_string(n_evals) + " evaluations read " + std::to_string(n_evals + d.T - 1) + " frames, " +
                                                     std::to_string(n_frames) + " given");
    if (n_frames > ((int64_t)1 << 40) / d.F) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_frames x bins is above 2^40");
    if (*row_stride == 0) *row_stride = n_frames * d.F;
    if (*row_stride < n_frames * d.F)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "row_stride " + std::to_string(*row_stride) + " is below the " + std::to_string(n_frames * d.F) + " elements of a row");
    return SYLDET_OK;
}

int tiles_arg(const syldet_trainer *t, int64_t n_evals)
{
    if ((int64_t)t->bank.channels * ((n_evals + t->desc.tile - 1) / t->desc.tile) > 0x7fffffff) return fail(SYLDET_ERR_UNSUPPORTED, "more than 2^31 - 1 tiles");
    return SYLDET_OK;
}

int adam_args(int64_t step, double lr, double beta1, double beta2, double eps)
{
    const char *why = sd::train_adam_refusal(step, lr, beta1, beta2, eps);
    return why ? fail(SYLDET_ERR_INVALID_ARGUMENT, why) : SYLDET_OK;
}

}  // namespace

extern "C" {

int syldet_train_param_count(const syldet_config_t *cfg, int64_t *n_params)
{
    if (!cfg || !n_params) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    int I = 0, H = 0, O = 0;
    if (int st = two_layers(*cfg, &I, &H, &O)) return st;
    *n_params = (int64_t)H * I + H + (int64_t)O * H + O;
    return SYLDET_OK;
}

// Both creations.  cfgs: the N networks' configurations, cfgs[0] the bank's own; multi: the trainer runs the multi form (also at N = 1).
static int trainer_create(const syldet_t *h, const syldet_recordings_t *r, const std::vector<const syldet_config_t *> &cfgs, bool multi, syldet_trainer_t **out)
{
    const syldet_config_t &c = *cfgs[0];
    const int N = (int)cfgs.size();
    int I = 0, H = 0, O = 0;
    for (int n = 0; n < N; n++) {
        const syldet_config_t &cn = *cfgs[(size_t)n];
        int In = 0, Hn = 0, On = 0;
        if (int st = two_layers(cn, &In, &Hn, &On)) return st;
        if (Hn > SYLDET_TRAIN_MAX_HIDDEN || On > SYLDET_TRAIN_MAX_OUTPUTS)
            return fail(SYLDET_ERR_UNSUPPORTED, "the trainer takes up to " + std::to_string(SYLDET_TRAIN_MAX_HIDDEN) + " hidden units and " +
                                                    std::to_string(SYLDET_TRAIN_MAX_OUTPUTS) + " outputs (" + std::to_string(Hn) + " and " + std::to_string(On) + " given)");
        if (cn.n_input_fns > sd::kMaxFns || cn.n_output_fns > sd::kMaxFns) return fail(SYLDET_ERR_UNSUPPORTED, "more than 8 processing functions");
        if (n == 0) {
            I = In;
            H = Hn;
            O = On;
            continue;
        }
        // (what syldet_config_compatible guarantees of a multi-network bank, checked where the kernel relies on it)
        bool same = In == I && Hn == H && On == O && cn.scaling == c.scaling && cn.n_input_fns == c.n_input_fns && cn.n_output_fns == c.n_output_fns &&
                    cn.layers[0].transfer == c.layers[0].transfer && cn.layers[1].transfer == c.layers[1].transfer;
        for (int k = 0; same && k < c.n_input_fns; k++) same = cn.input_fns[k].kind == c.input_fns[k].kind;
        for (int k = 0; same && k < c.n_output_fns; k++) same = cn.output_fns[k].kind == c.output_fns[k].kind;
        if (!same) return fail(SYLDET_ERR_UNSUPPORTED, "network " + std::to_string(n) + " differs from network 0 in shape, scaling, transfer or chain");
    }
    sd::BankInfo b{};
    sd::bank_info(h, &b);
    sd::TrainDesc d{};
    d.F = b.geom.bins;
    d.T = b.time_range;
    d.I = I;
    d.H = H;
    d.O = O;
    d.tf0 = c.layers[0].transfer;
    d.tf1 = c.layers[1].transfer;
    d.scaling = c.scaling;
    d.n_in_fns = c.n_input_fns;
    d.n_out_fns = c.n_output_fns;
    if (I != b.geom.inputs || O != b.geom.outputs || !sd::train_plan(d))
        return fail(SYLDET_ERR_UNSUPPORTED, "a network of " + std::to_string(I) + " inputs (" + std::to_string(d.F) + " bins x " + std::to_string(d.T) +
                                                " columns) does not fit the gradient kernel's local memory");
    const int P = sd::train_param_count(I, H, O);
    if ((int64_t)N * P > 0x7fffffff) return fail(SYLDET_ERR_UNSUPPORTED, "more than 2^31 - 1 parameters in all");
    if (N > 65535) return fail(SYLDET_ERR_UNSUPPORTED, "more than 65535 networks (the network is a launch's grid.y)");

    std::unique_ptr<syldet_trainer, int (*)(syldet_trainer_t *)> t(nullptr, syldet_trainer_destroy);
    std::vector<float> maps;
    std::vector<sd::DetSpan> by_row;
    std::vector<int32_t> row_begin, sorted_rows, net_row_begin;
    try {
        t.reset(new syldet_trainer());
        if (int st = t->read(h, r, sd::kSpanEvals)) return st;
        auto push = [&maps](const float *p, int n) {
            const int at = (int)maps.size();
            maps.insert(maps.end(), p, p + n);
            return at;
        };
        // every network's maps in a block of its own, laid out alike: the offsets below are into the network's block
        for (int n = 0; n < N; n++) {
            const syldet_config_t &cn = *cfgs[(size_t)n];
            sd::TrainDesc dn = d;
            const int base = (int)maps.size();
            for (int k = 0; k < cn.n_input_fns; k++) {
                const syldet_fn_t &f = cn.input_fns[k];
                dn.in_fns[k].kind = f.kind;
                dn.in_fns[k].y = f.y;
                if (f.kind >= SYLDET_FN_MAPMINMAX) {
                    dn.in_fns[k].xoff = push(f.x_offsets, I) - base;
                    dn.in_fns[k].gain = push(f.gains, I) - base;
                }
            }
            for (int k = 0; k < cn.n_output_fns; k++) {
                const syldet_fn_t &f = cn.output_fns[k];
                dn.out_fns[k].kind = f.kind;
                dn.out_fns[k].y = f.y;
                dn.out_fns[k].xoff = push(f.x_offsets, O) - base;
                dn.out_fns[k].gain = push(f.gains, O) - base;
            }
            t->maps_per = (int)maps.size() - base;
            t->descs.push_back(dn);
        }
        t->row_net.assign((size_t)b.channels, 0);
        if (N > 1 && b.channel_net) t->row_net.assign(b.channel_net, b.channel_net + b.channels);
        t->net_rows.assign((size_t)N, 0);
        for (int32_t n : t->row_net) t->net_rows[(size_t)n]++;
        net_row_begin.assign((size_t)N + 1, 0);
        for (int n = 0; n < N; n++) net_row_begin[(size_t)n + 1] = net_row_begin[(size_t)n] + t->net_rows[(size_t)n];
        sorted_rows.assign((size_t)b.channels, 0);
        {
            std::vector<int32_t> at(net_row_begin.begin(), net_row_begin.end() - 1);
            for (int32_t row = 0; row < b.channels; row++) sorted_rows[(size_t)at[(size_t)t->row_net[(size_t)row]]++] = row;
        }
        t->begin.assign((size_t)t->D + 1, 0);
        if (r) sd::spans_by_row(t->spans, b.channels, &by_row, &row_begin);     // what the targets kernel searches
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    t->multi = multi;
    t->N = N;
    t->P = P;
    t->row_frames = r ? sd::span_row_units(b, sd::kSpanFrames, t->row_samples, t->row_evals) : 0;
    if (r && t->row_evals > 0 && t->row_frames < t->row_evals + d.T - 1) return fail(SYLDET_ERR_INVALID_ARGUMENT, "the packed rows hold fewer frames than their evaluations read");

    sd::Carver blob;
    const size_t at_maps = blob.take(bytes_of(maps)), at_dets = blob.take(bytes_of(by_row)), at_rows = blob.take(bytes_of(row_begin)),
                 at_descs = blob.take(multi ? bytes_of(t->descs) : 0), at_sorted = blob.take(multi ? bytes_of(sorted_rows) : 0),
                 at_begin = blob.take(multi ? bytes_of(net_row_begin) : 0);
    SYLDET_HIP(hipSetDevice(b.device));
    SYLDET_HIP(sd::train_prepare(d));
    if (multi) SYLDET_HIP(sd::train_prepare_multi(d));
    if (int st = t->d_fixed.reserve(blob.total + 16)) return st;
    if (int st = t->d_part.reserve((size_t)N * (size_t)d.max_groups * ((size_t)P + 2) * sizeof(double))) return st;
    if (int st = t->d_opt.reserve(16 * (size_t)N + 3 * (size_t)N * (size_t)P * sizeof(float))) return st;
    char *base = (char *)t->d_fixed.ptr;
    SYLDET_HIP(upload(base, at_maps, maps));
    SYLDET_HIP(upload(base, at_dets, by_row));
    SYLDET_HIP(upload(base, at_rows, row_begin));
    for (int n = 0; n < N; n++) t->descs[(size_t)n].maps = (const float *)(base + at_maps) + (size_t)n * (size_t)t->maps_per;
    d = t->descs[0];
    t->d_dets = r ? (const sd::DetSpan *)(base + at_dets) : nullptr;
    t->d_row_begin = r ? (const int32_t *)(base + at_rows) : nullptr;
    if (multi) {
        t->descs_at = at_descs;
        SYLDET_HIP(upload(base, at_descs, t->descs));
        SYLDET_HIP(upload(base, at_sorted, sorted_rows));
        SYLDET_HIP(upload(base, at_begin, net_row_begin));
        t->mu.descs = (const sd::TrainDesc *)(base + at_descs);
        t->mu.rows = (const int32_t *)(base + at_sorted);
        t->mu.net_row_begin = (const int32_t *)(base + at_begin);
        t->mu.n_nets = N;
        t->mu.max_rows = *std::max_element(t->net_rows.begin(), t->net_rows.end());
    }
    t->desc = d;
    t->map_at = sd::train_first_map(d);
    if (t->map_at >= 0) {
        try {
            for (int n = 0; n < N; n++) {
                const float *own = maps.data() + (size_t)n * (size_t)t->maps_per;
                t->map.insert(t->map.end(), own + d.in_fns[t->map_at].xoff, own + d.in_fns[t->map_at].xoff + I);
                t->map.insert(t->map.end(), own + d.in_fns[t->map_at].gain, own + d.in_fns[t->map_at].gain + I);
            }
        } catch (const std::bad_alloc &) {
            return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
        }
    }
    *out = t.release();
    return SYLDET_OK;
}

int syldet_trainer_create(const syldet_t *h, const syldet_recordings_t *r, syldet_trainer_t **out)
{
    if (!out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (h->n_nets != 1 || !h->classes.empty() || h->root)
        return fail(SYLDET_ERR_UNSUPPORTED, "the trainer takes a plain bank: one network, not a multi-network or mixed one");
    try {
        return trainer_create(h, r, std::vector<const syldet_config_t *>{&h->cfg.view}, false, out);
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
}

int syldet_trainer_create_multi(const syldet_t *h, const syldet_recordings_t *r, syldet_trainer_t **out)
{
    if (!out) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (!h->classes.empty() || h->root) return fail(SYLDET_ERR_UNSUPPORTED, "the multi trainer takes a plain or a multi-network bank, not a mixed one");
    try {
        std::vector<const syldet_config_t *> cfgs;
        if (h->n_nets == 1) cfgs.push_back(&h->cfg.view);
        else if ((int)h->net_cfgs.size() == h->n_nets)
            for (const auto &own : h->net_cfgs) cfgs.push_back(&own->view);
        else return fail(SYLDET_ERR_UNSUPPORTED, "the bank does not keep its networks' configurations");
        return trainer_create(h, r, cfgs, true, out);
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
}

int syldet_trainer_destroy(syldet_trainer_t *t)
{
    if (!t) return SYLDET_OK;
    if (t->d_fixed.ptr || t->d_part.ptr || t->d_labels.ptr || t->d_opt.ptr) (void)hipSetDevice(t->bank.device);
    t->d_fixed.release();
    t->d_part.release();
    t->d_opt.release();
    t->d_labels.release();
    delete t;
    return SYLDET_OK;
}

int syldet_trainer_shape(const syldet_trainer_t *t, int32_t *n_detectors, int64_t *n_params, int32_t *n_out, int32_t *tile)
{
    if (!t) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_detectors) *n_detectors = t->D;
    if (n_params) *n_params = t->P;
    if (n_out) *n_out = t->desc.O;
    if (tile) *tile = t->desc.tile;
    return SYLDET_OK;
}

int syldet_trainer_networks(const syldet_trainer_t *t, int32_t *n_networks, int32_t *row_network)
{
    if (!t) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_networks) *n_networks = t->N;
    if (row_network) std::copy(t->row_net.begin(), t->row_net.end(), row_network);
    return SYLDET_OK;
}

int syldet_trainer_groups(const syldet_trainer_t *t, int64_t n_evals, int32_t *groups)
{
    if (!t || !groups) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_evals < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_evals is negative");
    if (int st = tiles_arg(t, n_evals)) return st;
    for (int n = 0; n < t->N; n++) groups[n] = sd::train_groups(t->desc, t->net_rows[(size_t)n], n_evals);
    return SYLDET_OK;
}

int syldet_train_targets_device(syldet_trainer_t *t, const int64_t *labels, const int64_t *label_begin, const int32_t *label_output,
                                int64_t half_width_samples, float weight_positive, float weight_negative, int64_t n_evals, float *d_targets,
                                float *d_weights, void *hip_stream)
{
    if (!t) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (!label_begin) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL label_begin");
    if (label_begin[0] != 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "label_begin[0] must be 0");
    for (int d = 0; d < t->D; d++)
        if (label_begin[d + 1] < label_begin[d]) return fail(SYLDET_ERR_INVALID_ARGUMENT, "label_begin[" + std::to_string(d + 1) + "] decreases");
    const int64_t n_labels = label_begin[t->D];
    if (n_labels > 0 && !labels) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL labels");
    for (int d = 0; d < t->D; d++)
        for (int64_t j = label_begin[d]; j + 1 < label_begin[d + 1]; j++)
            if (labels[j + 1] < labels[j])
                return fail(SYLDET_ERR_INVALID_ARGUMENT, "detector " + std::to_string(d) + ": label " + std::to_string(j + 1 - label_begin[d]) + " is not sorted");
    if (int st = outputs_arg(label_output, n_labels, t->desc.O)) return st;
    if (int st = half_width_arg(half_width_samples)) return st;
    if (int st = class_weights(weight_positive, weight_negative)) return st;
    if (n_evals < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_evals is negative");
    if (int st = t->row_units_arg(n_evals, "n_evals", "evaluations")) return st;
    if (n_evals > ((int64_t)1 << 31)) return fail(SYLDET_ERR_UNSUPPORTED, "more than 2^31 evaluations a row");
    const int rows = t->bank.channels;
    if (n_evals > 0 && rows > 0 && (!d_targets || !d_weights)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    SYLDET_HIP(hipSetDevice(t->bank.device));
    const size_t nb = ((size_t)t->D + 1) * sizeof(int64_t), nl = (size_t)n_labels * sizeof(int64_t), no = (size_t)n_labels * sizeof(int32_t);
    sd::Carver blob;
    const size_t at_begin = blob.take(nb), at_labels = blob.take(nl), at_output = blob.take(no);
    const bool same = t->has_labels && std::memcmp(t->begin.data(), label_begin, nb) == 0 &&
                      (n_labels == 0 || std::memcmp(t->labels.data(), labels, nl) == 0) && t->has_output == (label_output != nullptr) &&
                      (!label_output || n_labels == 0 || std::memcmp(t->output.data(), label_output, no) == 0);
    if (!same) {
        // other labels than the kept ones (the first call always): behind the last call, one blocking copy
        if (t->has_labels) SYLDET_HIP(hipStreamSynchronize(t->last));
        t->has_labels = false;
        try {
            t->begin.assign(label_begin, label_begin + t->D + 1);
            t->labels.assign(labels, labels + n_labels);
            if (label_output) t->output.assign(label_output, label_output + n_labels);
            else t->output.clear();
        } catch (const std::bad_alloc &) {
            return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
        }
        if (int st = t->d_labels.reserve(blob.total + 16)) return st;
        SYLDET_HIP(upload(t->d_labels.ptr, at_begin, label_begin, nb));
        SYLDET_HIP(upload(t->d_labels.ptr, at_labels, labels, nl));
        if (label_output) SYLDET_HIP(upload(t->d_labels.ptr, at_output, label_output, no));
        t->has_output = label_output != nullptr;
        t->has_labels = true;
    }
    t->last = stream;
    if (n_evals == 0 || rows == 0) return SYLDET_OK;
    char *base = (char *)t->d_labels.ptr;
    sd::TrainTargetsDesc d{};
    d.dets = t->d_dets;
    d.row_begin = t->d_row_begin;
    d.label_begin = (const int64_t *)(base + at_begin);
    d.labels = (const int64_t *)(base + at_labels);
    d.label_output = label_output ? (const int32_t *)(base + at_output) : nullptr;
    d.rows = rows;
    d.n_out = t->desc.O;
    d.first_index = t->bank.geom.first_index;
    d.hop = t->bank.geom.hop;
    d.half_width = half_width_samples;
    d.weight_positive = weight_positive;
    d.weight_negative = weight_negative;
    t->h->prof_begin();
    KernelTimer timer(t->h, stream, "train_targets_kernel");
    SYLDET_HIP(sd::launch_train_targets(d, n_evals, d_targets, d_weights, stream));
    return SYLDET_OK;
}

int syldet_train_targets_host(const int64_t *labels, int64_t n_labels, const int32_t *label_output, int32_t n_out, int64_t half_width_samples,
                              float weight_positive, float weight_negative, int64_t first_index, int64_t hop, int64_t n_evals, float *targets,
                              float *weights)
{
    if (n_out < 1 || n_out > SYLDET_TRAIN_MAX_OUTPUTS) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_out must be in [1, " + std::to_string(SYLDET_TRAIN_MAX_OUTPUTS) + "]");
    if (n_labels < 0 || n_evals < 0 || (n_labels > 0 && !labels) || (n_evals > 0 && (!targets || !weights)))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "a NULL array or a negative count");
    for (int64_t j = 0; j + 1 < n_labels; j++)
        if (labels[j + 1] < labels[j]) return fail(SYLDET_ERR_INVALID_ARGUMENT, "label " + std::to_string(j + 1) + " is not sorted");
    if (int st = outputs_arg(label_output, n_labels, n_out)) return st;
    if (int st = half_width_arg(half_width_samples)) return st;
    if (int st = class_weights(weight_positive, weight_negative)) return st;
    if (hop < 1 || hop > ((int64_t)1 << 30) || n_evals > ((int64_t)1 << 31) || first_index <= -sd::kTrainIndexLimit / 2 || first_index >= sd::kTrainIndexLimit / 2)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "hop outside [1, 2^30], more than 2^31 evaluations, or first_index out of range");
    for (int64_t e = 0; e < n_evals; e++)
        sd::train_target_write(sd::train_target_mask(first_index + e * hop, labels, label_output, n_labels, half_width_samples), n_out, weight_positive,
                               weight_negative, targets + e * n_out, weights + e);
    return SYLDET_OK;
}

int syldet_train_gradient_device(syldet_trainer_t *t, const float *d_columns, int64_t n_frames, int64_t row_stride, const float *d_params,
                                 const float *d_targets, const float *d_weights, int64_t n_evals, double *d_loss, float *d_gradient, void *hip_stream)
{
    if (!t) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (!d_params || !d_loss || !d_gradient) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    const sd::TrainDesc &d = t->desc;
    if (int st = columns_args(t, n_evals, n_frames, &row_stride)) return st;
    const int rows = t->bank.channels;
    if (n_evals > 0 && rows > 0 && (!d_columns || !d_targets || !d_weights)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int st = tiles_arg(t, n_evals)) return st;
    hipStream_t stream = (hipStream_t)hip_stream;
    SYLDET_HIP(hipSetDevice(t->bank.device));
    t->last = stream;
    const int groups = sd::train_groups(d, rows, n_evals);
    t->h->prof_begin();
    {
        KernelTimer timer(t->h, stream, "train_gradient_kernel");
        if (t->multi)
            SYLDET_HIP(sd::launch_train_gradient_multi(d, t->mu, d_columns, row_stride, d_params, d_targets, d_weights, n_evals, (double *)t->d_part.ptr, stream));
        else
            SYLDET_HIP(sd::launch_train_gradient(d, d_columns, row_stride, rows, d_params, d_targets, d_weights, n_evals, (double *)t->d_part.ptr, stream));
    }
    KernelTimer timer(t->h, stream, "train_combine_kernel");
    if (t->multi) SYLDET_HIP(sd::launch_train_combine_multi(d, t->mu, n_evals, (const double *)t->d_part.ptr, d_loss, d_gradient, stream));
    else SYLDET_HIP(sd::launch_train_combine(d, groups, (const double *)t->d_part.ptr, d_loss, d_gradient, stream));
    return SYLDET_OK;
}

int syldet_train_input_range_device(syldet_trainer_t *t, const float *d_columns, int64_t n_frames, int64_t row_stride, const float *d_weights,
                                    int64_t n_evals, float *d_range, int64_t *d_count, void *hip_stream)
{
    if (!t) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (!d_range || !d_count) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int st = columns_args(t, n_evals, n_frames, &row_stride)) return st;
    const sd::TrainDesc &d = t->desc;
    const int rows = t->bank.channels;
    if (n_evals > 0 && rows > 0 && (!d_columns || !d_weights)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int st = tiles_arg(t, n_evals)) return st;
    if (t->map_at < 0) return fail(SYLDET_ERR_UNSUPPORTED, "the configuration has no mapminmax input function");
    hipStream_t stream = (hipStream_t)hip_stream;
    SYLDET_HIP(hipSetDevice(t->bank.device));
    t->last = stream;
    const int groups = sd::train_groups(d, rows, n_evals);
    t->h->prof_begin();
    {
        KernelTimer timer(t->h, stream, "train_range_kernel");
        if (t->multi) SYLDET_HIP(sd::launch_train_range_multi(d, t->mu, t->map_at, d_columns, row_stride, d_weights, n_evals, (double *)t->d_part.ptr, stream));
        else SYLDET_HIP(sd::launch_train_range(d, t->map_at, d_columns, row_stride, rows, d_weights, n_evals, (double *)t->d_part.ptr, stream));
    }
    KernelTimer timer(t->h, stream, "train_range_combine_kernel");
    if (t->multi) SYLDET_HIP(sd::launch_train_range_combine_multi(d, t->mu, n_evals, (const double *)t->d_part.ptr, d_range, d_count, stream));
    else SYLDET_HIP(sd::launch_train_range_combine(d, groups, (const double *)t->d_part.ptr, d_range, d_count, stream));
    return SYLDET_OK;
}

int syldet_trainer_set_input_map_of(syldet_trainer_t *t, int32_t net, const float *x_offsets, const float *gains, float y)
{
    if (!t) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (net < 0 || net >= t->N) return fail(SYLDET_ERR_INVALID_ARGUMENT, "net " + std::to_string(net) + " is outside [0, " + std::to_string(t->N) + ")");
    if (!x_offsets || !gains) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (t->map_at < 0) return fail(SYLDET_ERR_UNSUPPORTED, "the configuration has no mapminmax input function");
    if (std::isnan(y)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "y is NaN");
    const int I = t->desc.I;
    const sd::DevFn &fn = t->desc.in_fns[t->map_at];
    float *own = t->map.data() + 2 * (size_t)I * (size_t)net;
    // behind the last call, which may still read the old map: one blocking copy (x_offsets and gains lie side by side), and in the
    // multi form one more of the network's y in its TrainDesc
    SYLDET_HIP(hipSetDevice(t->bank.device));
    SYLDET_HIP(hipStreamSynchronize(t->last));
    std::copy(x_offsets, x_offsets + I, own);
    std::copy(gains, gains + I, own + I);
    SYLDET_HIP(hipMemcpy((char *)t->d_fixed.ptr + ((size_t)net * (size_t)t->maps_per + (size_t)fn.xoff) * sizeof(float), own, 2 * (size_t)I * sizeof(float),
                         hipMemcpyHostToDevice));
    t->descs[(size_t)net].in_fns[t->map_at].y = y;
    if (net == 0) t->desc.in_fns[t->map_at].y = y;
    if (t->multi) {
        const size_t at = t->descs_at + (size_t)net * sizeof(sd::TrainDesc) + offsetof(sd::TrainDesc, in_fns) + (size_t)t->map_at * sizeof(sd::DevFn) + offsetof(sd::DevFn, y);
        SYLDET_HIP(hipMemcpy((char *)t->d_fixed.ptr + at, &y, sizeof(float), hipMemcpyHostToDevice));
    }
    return SYLDET_OK;
}

int syldet_trainer_input_map_of(const syldet_trainer_t *t, int32_t net, int32_t *index, float *x_offsets, float *gains, float *y)
{
    if (!t) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (net < 0 || net >= t->N) return fail(SYLDET_ERR_INVALID_ARGUMENT, "net " + std::to_string(net) + " is outside [0, " + std::to_string(t->N) + ")");
    if (t->map_at < 0) return fail(SYLDET_ERR_UNSUPPORTED, "the configuration has no mapminmax input function");
    const int I = t->desc.I;
    const float *own = t->map.data() + 2 * (size_t)I * (size_t)net;
    if (index) *index = t->map_at;
    if (x_offsets) std::copy(own, own + I, x_offsets);
    if (gains) std::copy(own + I, own + 2 * I, gains);
    if (y) *y = t->descs[(size_t)net].in_fns[t->map_at].y;
    return SYLDET_OK;
}

int syldet_trainer_set_input_map(syldet_trainer_t *t, const float *x_offsets, const float *gains, float y)
{
    return syldet_trainer_set_input_map_of(t, 0, x_offsets, gains, y);
}

int syldet_trainer_input_map(const syldet_trainer_t *t, int32_t *index, float *x_offsets, float *gains, float *y)
{
    return syldet_trainer_input_map_of(t, 0, index, x_offsets, gains, y);
}

int syldet_train_adam_device(syldet_trainer_t *t, float *d_params, const double *d_loss, const float *d_gradient, int64_t step, double lr, double beta1,
                             double beta2, double eps, double *d_mean_loss, void *hip_stream)
{
    if (!t) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (!d_params || !d_loss || !d_gradient) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int st = adam_args(step, lr, beta1, beta2, eps)) return st;
    hipStream_t stream = (hipStream_t)hip_stream;
    SYLDET_HIP(hipSetDevice(t->bank.device));
    t->last = stream;
    const size_t NP = (size_t)t->N * (size_t)t->P;
    float *m = (float *)((char *)t->d_opt.ptr + 16 * (size_t)t->N) + NP, *v = m + NP;
    t->h->prof_begin();
    KernelTimer timer(t->h, stream, "train_adam_kernel");
    if (t->multi)
        SYLDET_HIP(sd::launch_train_adam_multi(sd::train_adam_consts(step, lr, beta1, beta2, eps), t->P, t->N, d_loss, d_gradient, m, v, d_params, d_mean_loss, stream));
    else SYLDET_HIP(sd::launch_train_adam(sd::train_adam_consts(step, lr, beta1, beta2, eps), t->P, d_loss, d_gradient, m, v, d_params, d_mean_loss, stream));
    return SYLDET_OK;
}

int syldet_train_fit_device(syldet_trainer_t *t, const float *d_columns, int64_t n_frames, int64_t row_stride, const float *d_targets, const float *d_weights,
                            int64_t n_evals, float *d_params, int64_t steps, double lr, double beta1, double beta2, double eps, double *d_history,
                            void *hip_stream)
{
    if (!t) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    if (!d_params) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (steps < 0 || steps > ((int64_t)1 << 31)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "steps must be in [0, 2^31]");
    if (steps > 0 && !d_history) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL d_history");
    if (int st = adam_args(1, lr, beta1, beta2, eps)) return st;
    if (int st = columns_args(t, n_evals, n_frames, &row_stride)) return st;
    const sd::TrainDesc &d = t->desc;
    const int rows = t->bank.channels;
    if (n_evals > 0 && rows > 0 && (!d_columns || !d_targets || !d_weights)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int st = tiles_arg(t, n_evals)) return st;
    hipStream_t stream = (hipStream_t)hip_stream;
    SYLDET_HIP(hipSetDevice(t->bank.device));
    t->last = stream;
    const int groups = sd::train_groups(d, rows, n_evals);
    double *loss = (double *)t->d_opt.ptr;
    const size_t NP = (size_t)t->N * (size_t)t->P;
    float *grad = (float *)((char *)t->d_opt.ptr + 16 * (size_t)t->N), *m = grad + NP, *v = m + NP;
    for (int64_t k = 1; k <= steps; k++) {
        t->h->prof_begin();                                // (a step is a call of the profile: three kernels)
        {
            KernelTimer timer(t->h, stream, "train_gradient_kernel");
            if (t->multi)
                SYLDET_HIP(sd::launch_train_gradient_multi(d, t->mu, d_columns, row_stride, d_params, d_targets, d_weights, n_evals, (double *)t->d_part.ptr, stream));
            else
                SYLDET_HIP(sd::launch_train_gradient(d, d_columns, row_stride, rows, d_params, d_targets, d_weights, n_evals, (double *)t->d_part.ptr, stream));
        }
        {
            KernelTimer timer(t->h, stream, "train_combine_kernel");
            if (t->multi) SYLDET_HIP(sd::launch_train_combine_multi(d, t->mu, n_evals, (const double *)t->d_part.ptr, loss, grad, stream));
            else SYLDET_HIP(sd::launch_train_combine(d, groups, (const double *)t->d_part.ptr, loss, grad, stream));
        }
        KernelTimer timer(t->h, stream, "train_adam_kernel");
        if (t->multi)
            SYLDET_HIP(sd::launch_train_adam_multi(sd::train_adam_consts(k, lr, beta1, beta2, eps), t->P, t->N, loss, grad, m, v, d_params, d_history + (k - 1) * t->N,
                                                   stream));
        else SYLDET_HIP(sd::launch_train_adam(sd::train_adam_consts(k, lr, beta1, beta2, eps), t->P, loss, grad, m, v, d_params, d_history + (k - 1), stream));
    }
    return SYLDET_OK;
}

}  // extern "C"
