// LayerNorm / RMSNorm, dropout (counter RNG, rng.h) and cross entropy.
#include "binding/common.h"

namespace k8s_amd::binding {
namespace {

Tensor dropout(Tensor x, Tensor state, int64_t thr, double scale, int64_t site) {
  check_bf16_dense(x, -1, "x");
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) % 8 == 0, "dropout row length must be a multiple of 8");
  const k8s_amd::DropArgs dr = drop_args(state, thr, scale, site);
  const int D = (int)x.size(-1);
  auto y = torch::empty_like(x);
  if (x.numel()) launch_dropout(cbf(x), bf(y), x.numel() / D, D, dr, cur_stream());
  return y;
}
Tensor dropout_mask(Tensor state, int64_t thr, int64_t site, int64_t row0, int64_t R, int64_t C) {
  TORCH_CHECK(R >= 0 && C >= 0 && C <= 0x7fffffffLL && row0 >= 0, "bad mask shape");
  const k8s_amd::DropArgs dr = drop_args(state, thr, 1.0, site);
  auto out = torch::empty({R, C}, state.options().dtype(at::kByte));
  launch_dropout_mask(out.data_ptr<uint8_t>(), row0, R, (int)C, dr, cur_stream());
  return out;
}

// ------------------------------------------------------------------ layernorm / rmsnorm
// drop_state (optional, with res, LayerNorm only): xsum = bf16(keep * scale * x + res), see launch_norm_bwd
std::vector<Tensor> norm_fwd(Tensor x, OptTensor res, Tensor gamma, OptTensor beta, double eps, bool rms,
                             OptTensor drop_state, int64_t drop_thr, double drop_scale, int64_t drop_site) {
  check_bf16_dense(x, -1, "x");
  k8s_amd::DropArgs dr;
  if (drop_state) {
    TORCH_CHECK(res.has_value() && !rms, "dropout in norm_fwd needs LayerNorm with a residual");
    dr = drop_args(*drop_state, drop_thr, drop_scale, drop_site);
  }
  TORCH_CHECK(x.dim() >= 1, "x: rows of D");
  const int D = (int)x.size(-1);
  TORCH_CHECK(D > 0 && D % 8 == 0 && D <= 8192, "norm row length must be a multiple of 8 and <= 8192");
  const long R = x.numel() / D;
  check_channel_f32(gamma, D, "gamma");
  TORCH_CHECK(rms || beta.has_value(), "layernorm needs beta");
  if (beta) check_channel_f32(*beta, D, "beta");
  if (res) {
    check_bf16_dense(*res, -1, "res");
    TORCH_CHECK(res->sizes() == x.sizes(), "residual shape mismatch");
  }
  auto y = torch::empty_like(x);
  Tensor xsum = res ? torch::empty_like(x) : Tensor();
  auto mean = torch::empty({rms ? 1 : R}, gamma.options());
  auto rstd = torch::empty({R}, gamma.options());
  if (R == 0) return {y, mean, rstd, xsum};  // no rows: nothing to launch
  launch_norm_fwd(rms, cbf(x), res ? cbf(*res) : nullptr, res ? bf(xsum) : nullptr, f32(gamma), optf(beta), bf(y),
                  f32(mean), f32(rstd), R, D, (float)eps, cur_stream(), drop_state ? &dr : nullptr);
  return {y, mean, rstd, xsum};
}

// dsum (optional, fp32 [D]): also the column sums of dx -- the bias gradient of the linear that produced x's
// first summand (no residual gradient allowed)
// drop: the forward's dropout arguments; then (dx, da): `da` receives keep * scale * dx (the gradient of the dropped
// summand, while dx is the residual's) and dsum holds the column sums of da
std::vector<Tensor> norm_bwd_impl(Tensor dy, Tensor x, Tensor gamma, Tensor mean, Tensor rstd, OptTensor dres,
                                  Tensor dgamma, OptTensor dbeta, bool rms, OptTensor dsum,
                                  const k8s_amd::DropArgs* drop) {
  check_bf16_dense(x, -1, "x");
  check_bf16_dense(dy, -1, "dy");
  TORCH_CHECK(dy.sizes() == x.sizes() && x.dim() >= 1 && x.size(-1) > 0, "dy / x: the same rows of D");
  const int D = (int)x.size(-1);
  TORCH_CHECK(D % 8 == 0 && D <= 8192, "norm row length must be a multiple of 8 and <= 8192");
  const long R = x.numel() / D;
  check_channel_f32(gamma, D, "gamma");
  check_channel_f32(dgamma, D, "dgamma");
  check_cuda(mean, "mean"); check_dtype(mean, at::kFloat, "mean");
  TORCH_CHECK(rms || mean.numel() == R, "mean: one per row");
  check_channel_f32(rstd, R, "rstd");
  TORCH_CHECK(rms || dbeta.has_value(), "layernorm needs dbeta");
  if (dbeta) check_channel_f32(*dbeta, D, "dbeta");
  if (dres) {
    check_bf16_dense(*dres, -1, "dres");
    TORCH_CHECK(dres->sizes() == x.sizes(), "dres: the shape of x");
  }
  if (dsum) {
    TORCH_CHECK(!dres, "dsum: no residual gradient");
    check_channel_f32(*dsum, D, "dsum");
  }
  auto dx = torch::empty_like(x);
  Tensor da = drop ? torch::empty_like(x) : Tensor();
  if (R == 0) {  // no rows: the sums over them are zero, nothing to launch
    dgamma.zero_();
    if (dbeta) dbeta->zero_();
    if (dsum) dsum->zero_();
    return {dx, da};
  }
  auto work = torch::empty({k8s_amd::norm_workspace_floats(R, D)}, gamma.options());
  launch_norm_bwd(rms, cbf(dy), cbf(x), f32(gamma), f32(mean), f32(rstd), dres ? cbf(*dres) : nullptr, bf(dx),
                  f32(dgamma), dbeta ? f32(*dbeta) : nullptr, f32(work), R, D, cur_stream(),
                  dsum ? f32(*dsum) : nullptr, drop, drop ? bf(da) : nullptr);
  return {dx, da};
}
Tensor norm_bwd(Tensor dy, Tensor x, Tensor gamma, Tensor mean, Tensor rstd, OptTensor dres, Tensor dgamma,
                OptTensor dbeta, bool rms, OptTensor dsum) {
  return norm_bwd_impl(dy, x, gamma, mean, rstd, dres, dgamma, dbeta, rms, dsum, nullptr)[0];
}

// (dx, da) of a LayerNorm whose forward ran with dropout on its first summand
std::vector<Tensor> norm_bwd_dropout(Tensor dy, Tensor x, Tensor gamma, Tensor mean, Tensor rstd, OptTensor dres,
                                     Tensor dgamma, Tensor dbeta, OptTensor dsum, Tensor drop_state, int64_t drop_thr,
                                     double drop_scale, int64_t drop_site) {
  const k8s_amd::DropArgs dr = drop_args(drop_state, drop_thr, drop_scale, drop_site);
  return norm_bwd_impl(dy, x, gamma, mean, rstd, dres, dgamma, dbeta, false, dsum, &dr);
}

// ------------------------------------------------------------------ cross entropy
// logits [R, V] bf16 / fp32 rows with unit column stride, labels int64 [R]; returns logits is bf16
bool check_xent(const Tensor& logits, const Tensor& labels) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.stride(1) == 1, "logits must be [R, V] row-major");
  TORCH_CHECK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat, "logits: bf16 or fp32");
  check_cuda(labels, "labels"); check_dtype(labels, at::kLong, "labels");
  TORCH_CHECK(labels.numel() == logits.size(0), "labels: one per row");
  return logits.scalar_type() == at::kBFloat16;
}
std::vector<Tensor> xent_fwd(Tensor logits, Tensor labels, int64_t ignore_index, double smoothing) {
  const bool is_bf16 = check_xent(logits, labels);
  const long R = logits.size(0), V = logits.size(1);
  auto opt = logits.options().dtype(at::kFloat);
  auto loss = torch::empty({R}, opt);
  auto lse = torch::empty({R}, opt);
  if (R == 0) return {loss, lse};
  launch_xent_fwd(logits.data_ptr(), is_bf16, labels.data_ptr<int64_t>(), R, V, logits.stride(0), f32(loss), f32(lse),
                  ignore_index, (float)smoothing, cur_stream());
  return {loss, lse};
}

// evaluation metrics: (loss[R] fp32, rank[R] int32) over the columns of `logits` (pass a [:, :valid] view for a
// padded vocabulary); rank = #{j : l[j] > l[y]} + #{j < y : l[j] == l[y]}, ignored rows loss 0 / rank V
std::vector<Tensor> xent_eval(Tensor logits, Tensor labels, int64_t ignore_index) {
  const bool is_bf16 = check_xent(logits, labels);
  const long R = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V > 0 && V < (1L << 24), "xent_eval: 0 < V < 2^24 (the rank is counted in fp32)");
  auto loss = torch::empty({R}, logits.options().dtype(at::kFloat));
  auto rank = torch::empty({R}, logits.options().dtype(at::kInt));
  launch_xent_eval(logits.data_ptr(), is_bf16, labels.data_ptr<int64_t>(), R, V, logits.stride(0), f32(loss),
                   rank.data_ptr<int>(), ignore_index, cur_stream());
  return {loss, rank};
}

// logits [R, Vpad] dense; classes are the first V columns; returns dlogits [R, Vpad] (pad columns zero)
Tensor xent_bwd(Tensor logits, Tensor labels, Tensor lse, Tensor dscale, int64_t ignore_index, double smoothing,
                int64_t V) {
  const bool is_bf16 = check_xent(logits, labels);
  TORCH_CHECK(logits.is_contiguous(), "xent_bwd expects dense logits");
  const long R = logits.size(0), Vpad = logits.size(1);
  TORCH_CHECK(V > 0 && V <= Vpad, "xent_bwd: 0 < V <= the padded width");
  check_channel_f32(lse, R, "lse");
  TORCH_CHECK(dscale.is_cuda() && (dscale.numel() == 1 || dscale.numel() == R), "dscale: a GPU scalar or one per row");
  auto d = dscale.to(at::kFloat).contiguous();
  auto dl = torch::empty({R, Vpad}, logits.options());  // the kernel zeroes the pad columns itself
  if (R == 0) return dl;
  launch_xent_bwd(logits.data_ptr(), is_bf16, labels.data_ptr<int64_t>(), f32(lse), f32(d), d.numel() == R, R, V, Vpad,
                  dl.data_ptr(), ignore_index, (float)smoothing, cur_stream());
  return dl;
}

}  // namespace

void bind_norm(pybind11::module_& m) {
  m.def("dropout", &dropout, "x"_a, "state"_a, "thr"_a, "scale"_a, "site"_a);
  m.def("dropout_mask", &dropout_mask, "state"_a, "thr"_a, "site"_a, "row0"_a, "rows"_a, "cols"_a);
  m.def("norm_fwd", &norm_fwd, "x"_a, "res"_a, "gamma"_a, "beta"_a, "eps"_a, "rms"_a, "drop_state"_a = py::none(),
        "drop_thr"_a = 0, "drop_scale"_a = 1.0, "drop_site"_a = 0);
  m.def("norm_bwd_dropout", &norm_bwd_dropout, "dy"_a, "x"_a, "gamma"_a, "mean"_a, "rstd"_a, "dres"_a, "dgamma"_a,
        "dbeta"_a, "dsum"_a, "drop_state"_a, "drop_thr"_a, "drop_scale"_a, "drop_site"_a);
  m.def("norm_bwd", &norm_bwd, "dy"_a, "x"_a, "gamma"_a, "mean"_a, "rstd"_a, "dres"_a, "dgamma"_a, "dbeta"_a, "rms"_a,
        "dsum"_a = py::none());
  m.def("xent_fwd", &xent_fwd);
  m.def("xent_bwd", &xent_bwd);
  m.def("xent_eval", &xent_eval, "logits"_a, "labels"_a, "ignore_index"_a = -100);
}

}  // namespace k8s_amd::binding
