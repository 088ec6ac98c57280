// Optimizers on the flat parameter store: SGD / Adam, the layer-wise LARS / LAMB passes and their work-item table,
// gradient clipping and the bf16 gradient transport.
#include "binding/common.h"

#include <algorithm>
#include <cmath>
#include <utility>

namespace k8s_amd::binding {
namespace {

const uint8_t* mask_ptr(const OptTensor& m, long n) {
  if (!m) return nullptr;
  TORCH_CHECK(m->is_cuda() && m->scalar_type() == at::kByte && m->is_contiguous(), "decay_mask must be uint8 GPU");
  TORCH_CHECK(m->numel() * 64 >= n, "decay_mask must have one byte per 64 elements");
  return m->data_ptr<uint8_t>();
}

// device fp32 [lr, step] read by the optimizer kernels instead of the host scalars (hipGraph replay)
const float* hyper_ptr(const OptTensor& h) {
  if (!h) return nullptr;
  check_cuda(*h, "hyper"); check_dtype(*h, at::kFloat, "hyper");
  TORCH_CHECK(h->numel() >= 2, "hyper must be a contiguous fp32 [lr, step] tensor");
  return h->data_ptr<float>();
}

// device fp32 clip factor (clip_factor); nullptr when absent
const float* clip_ptr(const OptTensor& t) {
  if (!t) return nullptr;
  check_cuda(*t, "scale_t"); check_dtype(*t, at::kFloat, "scale_t");
  TORCH_CHECK(t->numel() >= 1, "scale_t is empty");
  return t->data_ptr<float>();
}
float bias_correction(double beta, int64_t step) { return 1.f - std::pow((float)beta, (float)step); }

bool grad_is_bf16(const Tensor& g, long n) {
  check_cuda(g, "grad");
  TORCH_CHECK(g.scalar_type() == at::kFloat || g.scalar_type() == at::kBFloat16, "grad must be fp32 or bf16");
  TORCH_CHECK(g.numel() == n, "grad size mismatch");
  return g.scalar_type() == at::kBFloat16;
}
uint16_t* param_bf16_ptr(const OptTensor& pbf, long n) {
  if (!pbf) return nullptr;
  check_cuda(*pbf, "param_bf16"); check_dtype(*pbf, at::kBFloat16, "param_bf16");
  TORCH_CHECK(pbf->numel() == n, "param_bf16 size mismatch");
  return bf(*pbf);
}
void fused_sgd(Tensor p, Tensor mom, Tensor g, OptTensor pbf, OptTensor decay_mask, double lr, double mu, double wd,
               double scale, OptTensor scale_t, bool nesterov, bool first_step, OptTensor hyper) {
  const long n = p.numel();
  TORCH_CHECK(n % 4 == 0, "flat buffer length must be a multiple of 4");
  check_channel_f32(p, n, "param"); check_channel_f32(mom, n, "momentum");
  const bool gb = grad_is_bf16(g, n);
  launch_sgd(f32(p), f32(mom), g.data_ptr(), gb, param_bf16_ptr(pbf, n), n, mask_ptr(decay_mask, n), (float)lr,
             (float)mu, (float)wd, (float)scale, clip_ptr(scale_t), hyper_ptr(hyper), nesterov, first_step,
             cur_stream());
}
void fused_adam(Tensor p, Tensor m1, Tensor m2, Tensor g, OptTensor pbf, OptTensor decay_mask, double lr, double b1,
                double b2, double eps, double wd, double scale, OptTensor scale_t, int64_t step, bool decoupled,
                OptTensor hyper) {
  const long n = p.numel();
  TORCH_CHECK(n % 4 == 0, "flat buffer length must be a multiple of 4");
  check_channel_f32(p, n, "param"); check_channel_f32(m1, n, "exp_avg"); check_channel_f32(m2, n, "exp_avg_sq");
  const bool gb = grad_is_bf16(g, n);
  const float bc1 = bias_correction(b1, step), bc2 = bias_correction(b2, step);
  launch_adam(f32(p), f32(m1), f32(m2), g.data_ptr(), gb, param_bf16_ptr(pbf, n), n, mask_ptr(decay_mask, n), (float)lr,
              (float)b1, (float)b2, (float)eps, (float)wd, (float)scale, clip_ptr(scale_t), hyper_ptr(hyper), bc1, bc2,
              decoupled, cur_stream());
}
Tensor grad_sumsq(Tensor g) {
  TORCH_CHECK(g.numel() % 4 == 0, "grad length must be a multiple of 4");
  const bool gb = grad_is_bf16(g, g.numel());
  auto out = torch::zeros({2}, g.options().dtype(at::kFloat));
  launch_sumsq(g.data_ptr(), gb, g.numel(), f32(out), cur_stream());
  return out;
}

// stats: fp32 [sum of squares, non-finite count] (grad_sumsq)
Tensor clip_factor(Tensor stats, double max_norm) {
  check_cuda(stats, "stats"); check_dtype(stats, at::kFloat, "stats");
  TORCH_CHECK(stats.numel() >= 2, "stats must be fp32 [sum of squares, non-finite count]");
  auto f = torch::empty({1}, stats.options());
  launch_clip_factor(f32(stats), (float)max_norm, f32(f), cur_stream());
  return f;
}

// ------------------------------------------------------------------ layer-wise optimizers (LARS / LAMB)
// The work-item table of kernels/layerwise.hip, validated ONCE on the host against the buffer sizes it will index
// (the kernels trust it), then kept on the device: every launch below only has to compare buffer sizes with the
// sizes the table was validated for.
struct LayerTable {
  Tensor items;      // int64 [n_items][4] on the device
  Tensor seg_start;  // int32 [n_seg + 1] on the device
  int64_t n_items = 0, n_seg = 0, n_master = 0, n_state = 0;
};

LayerTable layer_table(Tensor items, int64_t n_master, int64_t n_state, int64_t n_seg, at::Device device) {
  TORCH_CHECK(!items.is_cuda() && items.scalar_type() == at::kLong && items.is_contiguous(),
              "items must be a contiguous int64 host tensor");
  TORCH_CHECK(items.dim() == 2 && items.size(1) == 4, "items must be [n, 4] {flat offset, state offset, length, segment}");
  TORCH_CHECK(device.is_cuda(), "the table lives on the GPU");
  TORCH_CHECK(n_master >= 0 && n_state >= 0 && n_seg >= 0 && n_seg < (1 << 30), "bad sizes");
  const int64_t n = items.size(0);
  TORCH_CHECK(n < (int64_t(1) << 30), "too many work items");
  const int64_t* e = items.data_ptr<int64_t>();
  std::vector<int32_t> start(n_seg + 1, 0);
  std::vector<std::pair<int64_t, int64_t>> flat(n), state(n);
  int64_t prev = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t off = e[4 * i], soff = e[4 * i + 1], len = e[4 * i + 2], seg = e[4 * i + 3];
    TORCH_CHECK(len > 0 && len <= k8s_amd::kLayerItemMax && len % 64 == 0, "item ", i, ": length ", len);
    TORCH_CHECK(off >= 0 && off % 64 == 0 && off + len <= n_master, "item ", i, ": flat range outside the buffers");
    TORCH_CHECK(soff >= 0 && soff % 64 == 0 && soff + len <= n_state, "item ", i, ": state range outside the state");
    TORCH_CHECK(seg >= prev && seg < n_seg, "item ", i, ": segments must be in [0, n_seg) and contiguous in the table");
    prev = seg;
    ++start[seg + 1];
    flat[i] = {off, len};
    state[i] = {soff, len};
  }
  for (int64_t s = 0; s < n_seg; ++s) start[s + 1] += start[s];
  for (auto* v : {&flat, &state}) {  // two items on the same elements would race
    std::sort(v->begin(), v->end());
    for (int64_t i = 1; i < n; ++i)
      TORCH_CHECK((*v)[i - 1].first + (*v)[i - 1].second <= (*v)[i].first, "work items overlap");
  }
  LayerTable t;
  t.items = items.to(device);
  t.seg_start = torch::from_blob(start.data(), {n_seg + 1}, at::kInt).clone().to(device);
  t.n_items = n; t.n_seg = n_seg; t.n_master = n_master; t.n_state = n_state;
  return t;
}
void check_f32(const LayerTable& tab, const Tensor& t, int64_t n, const char* name) {
  check_channel_f32(t, n, name);  // n: what the item table was built for
  check_aligned(t, name);
  TORCH_CHECK(t.device() == tab.items.device(), name, " is not on the item table's device");
}
const uint8_t* seg_flags(const LayerTable& tab, const Tensor& flags) {
  TORCH_CHECK(flags.is_cuda() && flags.scalar_type() == at::kByte && flags.is_contiguous() && flags.numel() == tab.n_seg,
              "flags must be uint8 GPU, one per segment");
  return flags.data_ptr<uint8_t>();
}
bool layer_grad_bf16(const LayerTable& tab, const Tensor& g) {
  check_aligned(g, "grad");
  return grad_is_bf16(g, tab.n_master);
}

// pass 1. m1 / m2: LAMB's moments (advanced here); both absent for LARS.
void layer_sums(const LayerTable& tab, Tensor p, OptTensor m1, OptTensor m2, Tensor g, Tensor flags, Tensor partial,
                double b1, double b2, double eps, double wd, double scale, OptTensor scale_t, int64_t step,
                OptTensor hyper) {
  const bool lamb = m1.has_value();
  TORCH_CHECK(lamb == m2.has_value(), "LAMB takes both moments, LARS neither");
  check_f32(tab, p, tab.n_master, "param");
  if (lamb) { check_f32(tab, *m1, tab.n_state, "exp_avg"); check_f32(tab, *m2, tab.n_state, "exp_avg_sq"); }
  check_f32(tab, partial, 2 * tab.n_items, "partial");
  const bool gb = layer_grad_bf16(tab, g);
  const float bc1 = bias_correction(b1, step), bc2 = bias_correction(b2, step);
  launch_layer_sums(tab.items.data_ptr<int64_t>(), (int)tab.n_items, f32(p), lamb ? f32(*m1) : nullptr,
                    lamb ? f32(*m2) : nullptr, g.data_ptr(), gb, seg_flags(tab, flags), f32(partial), lamb, (float)b1,
                    (float)b2, (float)eps, (float)wd, (float)scale, clip_ptr(scale_t), hyper_ptr(hyper), bc1, bc2,
                    cur_stream());
}
void layer_fold(const LayerTable& tab, Tensor partial, Tensor sums, OptTensor scale_t) {
  check_f32(tab, partial, 2 * tab.n_items, "partial");
  check_f32(tab, sums, 2 * tab.n_seg, "sums");
  launch_layer_fold(f32(partial), tab.seg_start.data_ptr<int32_t>(), (int)tab.n_seg, f32(sums), clip_ptr(scale_t),
                    cur_stream());
}
void layer_ratio(const LayerTable& tab, Tensor sums, Tensor flags, Tensor ratio, bool lamb, double eta, double wd,
                 OptTensor scale_t) {
  check_f32(tab, sums, 2 * tab.n_seg, "sums");
  check_f32(tab, ratio, tab.n_seg, "ratio");
  launch_layer_ratio(f32(sums), seg_flags(tab, flags), (int)tab.n_seg, f32(ratio), lamb, (float)eta, (float)wd,
                     clip_ptr(scale_t), cur_stream());
}

// pass 2. LARS: st1 = momentum, st2 absent. LAMB: st1 / st2 = the moments pass 1 advanced.
void layer_update(const LayerTable& tab, Tensor p, Tensor st1, OptTensor st2, Tensor g, OptTensor pbf, Tensor flags,
                  Tensor ratio, double lr, double mu, double b1, double b2, double eps, double wd, double scale,
                  OptTensor scale_t, int64_t step, bool first_step, OptTensor hyper) {
  const bool lamb = st2.has_value();
  check_f32(tab, p, tab.n_master, "param");
  check_f32(tab, st1, tab.n_state, lamb ? "exp_avg" : "momentum");
  if (lamb) check_f32(tab, *st2, tab.n_state, "exp_avg_sq");
  check_f32(tab, ratio, tab.n_seg, "ratio");
  const bool gb = layer_grad_bf16(tab, g);
  if (pbf) check_aligned(*pbf, "param_bf16");
  const float bc1 = bias_correction(b1, step), bc2 = bias_correction(b2, step);
  launch_layer_update(tab.items.data_ptr<int64_t>(), (int)tab.n_items, f32(p), f32(st1), lamb ? f32(*st2) : nullptr,
                      g.data_ptr(), gb, param_bf16_ptr(pbf, tab.n_master), seg_flags(tab, flags), f32(ratio), lamb,
                      (float)lr, (float)mu, (float)b1, (float)b2, (float)eps, (float)wd, (float)scale,
                      clip_ptr(scale_t), hyper_ptr(hyper), bc1, bc2, first_step, cur_stream());
}

// ------------------------------------------------------------------ bf16 gradient transport
// recv: bf16 [world * n] (all-to-all receive buffer of one bucket) -> fp32 out [n] and/or bf16 out_bf [n]
void slice_sum(Tensor recv, int64_t world, OptTensor out, OptTensor out_bf) {
  check_cuda(recv, "recv"); check_dtype(recv, at::kBFloat16, "recv");
  TORCH_CHECK(world > 0 && recv.numel() % world == 0, "recv must be [world * n]");
  const long n = recv.numel() / world;
  float* o = nullptr;
  uint16_t* ob = nullptr;
  if (out && out->defined()) {
    check_channel_f32(*out, n, "out");
    o = f32(*out);
  }
  if (out_bf && out_bf->defined()) {
    check_cuda(*out_bf, "out_bf"); check_dtype(*out_bf, at::kBFloat16, "out_bf");
    TORCH_CHECK(out_bf->numel() == n, "out_bf must be [n] bf16");
    ob = bf(*out_bf);
  }
  TORCH_CHECK(o || ob, "slice_sum: no output");
  launch_slice_sum(cbf(recv), n, (int)world, o, ob, cur_stream());
}
Tensor cast_bf16(Tensor x, OptTensor out) {
  check_cuda(x, "x"); check_dtype(x, at::kFloat, "x");
  if (out && out->defined()) {
    check_cuda(*out, "out"); check_dtype(*out, at::kBFloat16, "out");
    TORCH_CHECK(out->numel() == x.numel(), "out size mismatch");
  }
  Tensor o = (out && out->defined()) ? *out : torch::empty({x.numel()}, x.options().dtype(at::kBFloat16));
  launch_cast_bf16(f32(x), bf(o), x.numel(), cur_stream());
  return o;
}

// ------------------------------------------------------------------ gradient accumulation (kernels/accum.hip)
// Two flat fp32 buffers of one layout and the 64-aligned range [lo, hi) of them a pass works on. Returns hi - lo.
long check_accum_range(const Tensor& a, const char* a_name, const Tensor& b, const char* b_name, int64_t lo,
                       int64_t hi) {
  check_cuda(a, a_name); check_dtype(a, at::kFloat, a_name); check_aligned(a, a_name);
  check_channel_f32(b, a.numel(), b_name); check_aligned(b, b_name);
  TORCH_CHECK(a.device() == b.device(), a_name, " and ", b_name, " are on different devices");
  TORCH_CHECK(a.data_ptr() != b.data_ptr() || a.numel() == 0, a_name, " and ", b_name, " must be different buffers");
  TORCH_CHECK(a.numel() % 64 == 0, "flat buffer length must be a multiple of 64");
  TORCH_CHECK(lo % 64 == 0 && hi % 64 == 0, "range [", lo, ", ", hi, ") must be 64-aligned");
  TORCH_CHECK(0 <= lo && lo <= hi && hi <= a.numel(), "range [", lo, ", ", hi, ") is outside the ", a.numel(),
              " elements");
  return hi - lo;
}
void grad_accumulate(Tensor acc, Tensor g, int64_t lo, int64_t hi, bool first) {
  const long n = check_accum_range(acc, "acc", g, "grad", lo, hi);
  launch_grad_accumulate(f32(acc) + lo, f32(g) + lo, n, first, cur_stream());
}
void grad_fold(Tensor g, Tensor acc, int64_t lo, int64_t hi, OptTensor out_bf) {
  const long n = check_accum_range(g, "grad", acc, "acc", lo, hi);
  uint16_t* ob = nullptr;
  if (out_bf && out_bf->defined()) {
    check_bf16_dense(*out_bf, -1, "out_bf");
    TORCH_CHECK(out_bf->device() == g.device(), "out_bf is not on the gradient's device");
    TORCH_CHECK(out_bf->numel() >= n, "out_bf has ", out_bf->numel(), " elements, the range has ", n);
    ob = bf(*out_bf);
  }
  launch_grad_fold(f32(g) + lo, f32(acc) + lo, ob, n, cur_stream());
}

}  // namespace

void bind_optim(pybind11::module_& m) {
  m.def("fused_sgd", &fused_sgd, "p"_a, "mom"_a, "g"_a, "pbf"_a, "decay_mask"_a, "lr"_a, "mu"_a, "wd"_a, "scale"_a,
        "scale_t"_a, "nesterov"_a, "first_step"_a, "hyper"_a = py::none());
  m.def("fused_adam", &fused_adam, "p"_a, "m1"_a, "m2"_a, "g"_a, "pbf"_a, "decay_mask"_a, "lr"_a, "b1"_a, "b2"_a,
        "eps"_a, "wd"_a, "scale"_a, "scale_t"_a, "step"_a, "decoupled"_a, "hyper"_a = py::none());
  m.def("grad_sumsq", &grad_sumsq);
  m.def("clip_factor", &clip_factor);
  py::class_<LayerTable>(m, "LayerTable", "validated work-item table of the layer-wise optimizers")
      .def_readonly("items", &LayerTable::items).def_readonly("seg_start", &LayerTable::seg_start)
      .def_readonly("n_items", &LayerTable::n_items).def_readonly("n_seg", &LayerTable::n_seg)
      .def_readonly("n_master", &LayerTable::n_master).def_readonly("n_state", &LayerTable::n_state);
  m.def("layer_table", &layer_table, "items"_a, "n_master"_a, "n_state"_a, "n_seg"_a, "device"_a);
  m.def("layer_sums", &layer_sums, "table"_a, "p"_a, "m1"_a, "m2"_a, "g"_a, "flags"_a, "partial"_a, "b1"_a, "b2"_a,
        "eps"_a, "wd"_a, "scale"_a, "scale_t"_a, "step"_a, "hyper"_a = py::none());
  m.def("layer_fold", &layer_fold, "table"_a, "partial"_a, "sums"_a, "scale_t"_a);
  m.def("layer_ratio", &layer_ratio, "table"_a, "sums"_a, "flags"_a, "ratio"_a, "lamb"_a, "eta"_a, "wd"_a, "scale_t"_a);
  m.def("layer_update", &layer_update, "table"_a, "p"_a, "st1"_a, "st2"_a, "g"_a, "pbf"_a, "flags"_a, "ratio"_a, "lr"_a,
        "mu"_a, "b1"_a, "b2"_a, "eps"_a, "wd"_a, "scale"_a, "scale_t"_a, "step"_a, "first_step"_a,
        "hyper"_a = py::none());
  m.def("slice_sum", &slice_sum, "recv"_a, "world"_a, "out"_a = py::none(), "out_bf"_a = py::none(),
        "fp32 rank-order sum of an all-to-all's bf16 chunks");
  m.def("cast_bf16", &cast_bf16, "x"_a, "out"_a = py::none());
  m.def("grad_accumulate", &grad_accumulate, "acc"_a, "g"_a, "lo"_a, "hi"_a, "first"_a,
        "acc[lo:hi] = g[lo:hi] if first else acc[lo:hi] + g[lo:hi]");
  m.def("grad_fold", &grad_fold, "g"_a, "acc"_a, "lo"_a, "hi"_a, "out_bf"_a = py::none(),
        "g[lo:hi] += acc[lo:hi]; out_bf[:hi - lo] = bf16(g[lo:hi]) when given");
}

}  // namespace k8s_amd::binding
