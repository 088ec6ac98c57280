// BatchNorm (NHWC): forward / backward with their own reductions or with `sums` that come from a convolution's
// epilogue, the two-BatchNorm (ResNet downsample block) forms and the stem's BN + ReLU + max pool.
#include "binding/common.h"

namespace k8s_amd::binding {
namespace {

// x of a BatchNorm: dense bf16 with the channels last, in whole 16-byte groups of 8 channels (what every kernel reads
// and writes); returns C
int bn_channels(const Tensor& x, const char* name) {
  check_bf16_dense(x, -1, name);
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0, name, ": channels last");
  const int C = (int)x.size(-1);
  TORCH_CHECK(C % 8 == 0, "channels must be a multiple of 8");
  return C;
}
// gamma / beta / running mean / running variance
void check_affine(const Tensor& gamma, const Tensor& beta, const Tensor& run_mean, const Tensor& run_var, long C) {
  check_channel_f32(gamma, C, "gamma"); check_channel_f32(beta, C, "beta");
  check_channel_f32(run_mean, C, "run_mean"); check_channel_f32(run_var, C, "run_var");
}
// what every backward reads and writes per channel
void check_bwd_vectors(const Tensor& mean, const Tensor& invstd, const Tensor& gamma, const Tensor& beta,
                       const Tensor& dgamma, const Tensor& dbeta, long C) {
  check_channel_f32(mean, C, "mean"); check_channel_f32(invstd, C, "invstd");
  check_channel_f32(gamma, C, "gamma"); check_channel_f32(beta, C, "beta");
  check_channel_f32(dgamma, C, "dgamma"); check_channel_f32(dbeta, C, "dbeta");
}
void check_same_shape(const Tensor& t, const Tensor& x, const char* name) {
  check_bf16_dense(t, -1, name);
  TORCH_CHECK(t.sizes() == x.sizes(), name, " must have the shape of x");
}

// want_mask: also return the packed ReLU mask (uint8 [M*C/8], bit j of byte e = y[8e+j] > 0) for the backward
Tensor relu_mask_for(const Tensor& x, bool want_mask) {
  return want_mask ? torch::empty({x.numel() / 8}, x.options().dtype(at::kByte)) : Tensor();
}

// sums (optional): the statistics come from a convolution's epilogue sums instead of a reduction over x.
// want_sub2 (with sums): also y[:, ::2, ::2, :] (the next block's downsample input), written by the same pass
std::vector<Tensor> bn_fwd_impl(const Tensor& x, const OptTensor& res, const Tensor& gamma, const Tensor& beta,
                                const Tensor* sums, const Tensor& run_mean, const Tensor& run_var, bool training,
                                double momentum, double eps, bool relu, bool want_mask, bool want_sub2) {
  const int C = bn_channels(x, "x");
  const long M = x.numel() / C;
  check_affine(gamma, beta, run_mean, run_var, C);
  const int nrep = sums ? check_stat_sums(*sums, C, "sums", false) : 0;
  if (res) check_same_shape(*res, x, "res");
  TORCH_CHECK(!want_sub2 || x.dim() == 4, "want_sub2: contiguous NHWC x");
  auto y = torch::empty_like(x);
  auto mean = torch::empty({C}, gamma.options()), invstd = torch::empty({C}, gamma.options());
  auto params = torch::empty({2 * C}, gamma.options());
  Tensor mask = relu_mask_for(x, want_mask);
  uint8_t* mk = want_mask ? mask.data_ptr<uint8_t>() : nullptr;
  std::vector<Tensor> out = {y, mean, invstd};
  if (want_mask) out.push_back(mask);
  if (!sums) {
    Tensor work = training ? torch::empty({k8s_amd::bn_workspace_floats(M, C)}, gamma.options()) : mean;
    launch_bn_fwd(cbf(x), res ? cbf(*res) : nullptr, f32(gamma), f32(beta), bf(y), f32(mean), f32(invstd),
                  f32(run_mean), f32(run_var), f32(work), f32(params), M, C, (float)eps, (float)momentum, training,
                  relu, cur_stream(), mk);
    return out;
  }
  const int H = want_sub2 ? (int)x.size(1) : 1, W = want_sub2 ? (int)x.size(2) : 1;
  Tensor ysub = want_sub2 ? torch::empty({x.size(0), (H + 1) / 2, (W + 1) / 2, C}, x.options()) : Tensor();
  launch_bn_fwd_from_sums(cbf(x), res ? cbf(*res) : nullptr, f32(gamma), f32(beta), bf(y), f32(*sums), nrep, f32(mean),
                          f32(invstd), f32(run_mean), f32(run_var), f32(params), M, C, (float)eps, (float)momentum,
                          relu, cur_stream(), mk, want_sub2 ? bf(ysub) : nullptr, H, W);
  if (want_sub2) out.push_back(ysub);
  return out;
}
std::vector<Tensor> bn_fwd(Tensor x, OptTensor res, Tensor gamma, Tensor beta, Tensor run_mean, Tensor run_var,
                           bool training, double momentum, double eps, bool relu, bool want_mask) {
  return bn_fwd_impl(x, res, gamma, beta, nullptr, run_mean, run_var, training, momentum, eps, relu, want_mask, false);
}
std::vector<Tensor> bn_fwd_from_sums(Tensor x, OptTensor res, Tensor gamma, Tensor beta, Tensor sums, Tensor run_mean,
                                     Tensor run_var, double momentum, double eps, bool relu, bool want_mask,
                                     bool want_sub2) {
  return bn_fwd_impl(x, res, gamma, beta, &sums, run_mean, run_var, true, momentum, eps, relu, want_mask, want_sub2);
}

// y = relu(BN(x) + BN_r(xr)) with both BatchNorms' statistics from conv epilogue sums (ResNet downsample block:
// bn3 + the downsample BN in one apply pass). Returns (y, mean, invstd, packed ReLU mask, mean_r, invstd_r).
std::vector<Tensor> bn_fwd_from_sums_dual(Tensor x, Tensor sums, Tensor gamma, Tensor beta, Tensor run_mean,
                                          Tensor run_var, Tensor xr, Tensor sums_r, Tensor gamma_r, Tensor beta_r,
                                          Tensor run_mean_r, Tensor run_var_r, double momentum, double eps) {
  const int C = bn_channels(x, "x");
  const long M = x.numel() / C;
  check_same_shape(xr, x, "xr");
  check_affine(gamma, beta, run_mean, run_var, C);
  check_affine(gamma_r, beta_r, run_mean_r, run_var_r, C);
  const int nrep = check_stat_sums(sums, C, "sums", false), nrep_r = check_stat_sums(sums_r, C, "sums_r", false);
  auto y = torch::empty_like(x);
  auto mean = torch::empty({C}, gamma.options()), invstd = torch::empty({C}, gamma.options());
  auto mean_r = torch::empty({C}, gamma.options()), invstd_r = torch::empty({C}, gamma.options());
  auto params = torch::empty({2 * C}, gamma.options()), params_r = torch::empty({2 * C}, gamma.options());
  Tensor mask = relu_mask_for(x, true);
  launch_bn_fwd_from_sums_dual(cbf(x), f32(gamma), f32(beta), f32(sums), nrep, f32(mean), f32(invstd), f32(run_mean),
                               f32(run_var), f32(params), cbf(xr), f32(gamma_r), f32(beta_r), f32(sums_r), nrep_r,
                               f32(mean_r), f32(invstd_r), f32(run_mean_r), f32(run_var_r), f32(params_r), bf(y),
                               mask.data_ptr<uint8_t>(), M, C, (float)eps, (float)momentum, cur_stream());
  return {y, mean, invstd, mask, mean_r, invstd_r};
}

// BatchNorm statistics of a conv output from its epilogue sums, WITHOUT the apply pass: returns (mean, invstd,
// params = fp32 [2][C] scale | shift) for a consumer that normalises on load (conv_fwd / conv_wgrad / gemm xform).
std::vector<Tensor> bn_finalize(Tensor sums, Tensor gamma, Tensor beta, Tensor run_mean, Tensor run_var,
                                int64_t count, double momentum, double eps) {
  const int C = (int)gamma.numel();
  TORCH_CHECK(C > 0 && C % 8 == 0, "channels must be a multiple of 8");  // what every consumer of params loads
  check_affine(gamma, beta, run_mean, run_var, C);
  const int nrep = check_stat_sums(sums, C, "sums", false);
  auto mean = torch::empty({C}, gamma.options()), invstd = torch::empty({C}, gamma.options());
  auto params = torch::empty({2 * C}, gamma.options());
  launch_bn_finalize_sums(f32(gamma), f32(beta), f32(sums), nrep, f32(mean), f32(invstd), f32(run_mean), f32(run_var),
                          f32(params), (long)count, C, (float)eps, (float)momentum, cur_stream());
  return {mean, invstd, params};
}

// ResNet stem: BatchNorm (statistics from the conv epilogue sums) + ReLU + 3x3 / s2 / p1 max pool in one pass; the
// BN output is never stored. Returns (pooled y, winner idx, mean, invstd); with `want_link` also (xarg, ybits): the
// winner's x and packed ReLU bits per pooled element (the BatchNorm-backward sums in the consumers' dgrad epilogues).
std::vector<Tensor> bn_relu_maxpool(Tensor x, Tensor sums, Tensor gamma, Tensor beta, Tensor run_mean, Tensor run_var,
                                    double momentum, double eps, bool want_link) {
  check_bf16_dense(x, 4, "x");
  const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  TORCH_CHECK(C > 0 && C % 8 == 0 && 256 % (C / 8) == 0, "C / 8 must divide 256");
  check_affine(gamma, beta, run_mean, run_var, C);
  const int nrep = check_stat_sums(sums, C, "sums", false);
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  auto y = torch::empty({N, Ho, Wo, C}, x.options());
  auto idx = torch::empty({N, Ho, Wo, C}, x.options().dtype(at::kByte));
  auto mean = torch::empty({C}, gamma.options()), invstd = torch::empty({C}, gamma.options());
  auto params = torch::empty({2 * C}, gamma.options());
  Tensor xarg, ybits;
  if (want_link) {
    xarg = torch::empty({N, Ho, Wo, C}, x.options());
    ybits = torch::empty({(long)N * Ho * Wo * C / 8}, x.options().dtype(at::kByte));
  }
  launch_bn_relu_maxpool_fwd(cbf(x), f32(gamma), f32(beta), f32(sums), nrep, f32(mean), f32(invstd), f32(run_mean),
                             f32(run_var), f32(params), bf(y), idx.data_ptr<uint8_t>(), N, H, W, C, (float)eps,
                             (float)momentum, cur_stream(), want_link ? bf(xarg) : nullptr,
                             want_link ? ybits.data_ptr<uint8_t>() : nullptr);
  if (want_link) return {y, idx, mean, invstd, xarg, ybits};
  return {y, idx, mean, invstd};
}

// One BatchNorm of a backward (launchers.h BnBwdSide) from its tensors, with the allocations it owns. sums (optional):
// the reduction was already done by dy's producer (a data gradient's epilogue), leaving the final and apply passes --
// and no workspace is allocated. pool: the stem's BN + max pool (its own workspace size; sums of exactly
// conv_stat_replicas). s.dx stays null (a deferred apply pass) until the caller sets it.
struct BwdSide {
  k8s_amd::BnBwdSide s;
  int nrep = 0;
  Tensor params, work;
};
BwdSide bwd_side(const Tensor& x, const Tensor& mean, const Tensor& invstd, const Tensor& gamma, const Tensor& beta,
                 const Tensor& dgamma, const Tensor& dbeta, const Tensor* sums, const char* sums_name, long M, int C,
                 bool pool = false) {
  check_bwd_vectors(mean, invstd, gamma, beta, dgamma, dbeta, C);
  BwdSide b;
  if (sums) b.nrep = check_stat_sums(*sums, C, sums_name, pool);
  b.params = torch::empty({4 * C}, gamma.options());
  if (!sums)
    b.work = torch::empty({pool ? k8s_amd::pool_bn_workspace_floats(C) : k8s_amd::bn_workspace_floats(M, C)},
                          gamma.options());
  b.s.x = cbf(x);
  b.s.mean = f32(mean); b.s.invstd = f32(invstd); b.s.gamma = f32(gamma); b.s.beta = f32(beta);
  b.s.dgamma = f32(dgamma); b.s.dbeta = f32(dbeta);
  b.s.sums = sums ? f32(*sums) : nullptr;
  b.s.work = sums ? nullptr : f32(b.work);
  b.s.params = f32(b.params);
  return b;
}
const Tensor* opt_ptr(const OptTensor& t) { return t && t->defined() ? &*t : nullptr; }

// Backward of bn_relu_maxpool: dx of the conv output x [N, H, W, C] from dpool / idx [N, ceil(H/2), ceil(W/2), C];
// dgamma / dbeta written into the given fp32 tensors. sums (optional): the BatchNorm-backward sums already taken
// (fp32 [conv_stat_replicas, 2, C] over g = bit ? dpool : 0 at the winners' x, by the data gradients into the pooled
// output): the final and apply passes only.
Tensor pool_bn_bwd(Tensor dpool, Tensor idx, Tensor x, Tensor mean, Tensor invstd, Tensor gamma, Tensor beta,
                   Tensor dgamma, Tensor dbeta, OptTensor sums) {
  check_bf16_dense(x, 4, "x");
  check_bf16_dense(dpool, 4, "dpool");
  check_cuda(idx, "idx"); check_dtype(idx, at::kByte, "idx");
  const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  TORCH_CHECK(C > 0 && C % 8 == 0 && 256 % (C / 8) == 0, "C / 8 must divide 256");
  TORCH_CHECK(dpool.sizes() == idx.sizes() && dpool.size(0) == N && dpool.size(1) == (H + 1) / 2 &&
                  dpool.size(2) == (W + 1) / 2 && dpool.size(3) == C, "dpool / idx shape mismatch");
  BwdSide a = bwd_side(x, mean, invstd, gamma, beta, dgamma, dbeta, opt_ptr(sums), "sums", 0, C, true);
  auto dx = torch::empty_like(x);
  a.s.dx = bf(dx);
  launch_pool_bn_bwd(cbf(dpool), idx.data_ptr<uint8_t>(), a.nrep, a.s, N, H, W, C, cur_stream());
  return dx;
}

// (dx, dres or empty); writes dgamma / dbeta into the given (flat-bucket view) tensors. The ReLU of the forward comes
// from the packed `mask` (residual BN), is recomputed from x (`relu_x`), or -- given the BN output `y` -- is packed
// from y first (compatibility; the trainer passes the mask). sums (optional, with the mask or relu_x, not with y).
std::vector<Tensor> bn_bwd(Tensor dy, Tensor x, OptTensor y, Tensor mean, Tensor invstd, Tensor gamma, Tensor beta,
                           bool relu_x, Tensor dgamma, Tensor dbeta, bool want_dres, OptTensor mask, OptTensor sums) {
  const int C = bn_channels(x, "x");
  const long M = x.numel() / C;
  check_same_shape(dy, x, "dy");
  const bool has_mask = mask && mask->defined();
  TORCH_CHECK(!(relu_x && (y || has_mask)) && !(y && has_mask), "relu_x, y and the packed mask are exclusive");
  const Tensor* pre = opt_ptr(sums);
  TORCH_CHECK(!pre || has_mask || relu_x, "sums: with the packed mask or relu_x");
  TORCH_CHECK(!pre || !want_dres || has_mask, "sums with relu_x: no dres");
  const uint8_t* mk = has_mask ? check_bit_mask(*mask, x.numel(), "mask") : nullptr;
  BwdSide a = bwd_side(x, mean, invstd, gamma, beta, dgamma, dbeta, pre, "sums", M, C);
  Tensor ymask;
  if (y) {
    check_same_shape(*y, x, "y");
    TORCH_CHECK(x.numel() % 8 == 0, "y: a multiple of 8 elements to pack");
    ymask = relu_mask_for(x, true);
    launch_relu_mask(cbf(*y), ymask.data_ptr<uint8_t>(), x.numel() / 8, cur_stream());
    mk = ymask.data_ptr<uint8_t>();
  }
  auto dx = torch::empty_like(x);
  Tensor dres = want_dres ? torch::empty_like(x) : Tensor();
  a.s.dx = bf(dx);
  launch_bn_bwd_params(cbf(dy), mk, relu_x, a.nrep, a.s, nullptr, M, C, cur_stream());
  launch_bn_bwd_apply(cbf(dy), mk, relu_x, a.s, nullptr, want_dres ? bf(dres) : nullptr, M, C, cur_stream());
  return {dx, dres};
}

// The two halves of bn_bwd for a residual BatchNorm (packed mask), for a consumer of dx that applies the backward as it
// loads (bwd1x1_fused with x3 / mask / params). bn_bwd_params: dgamma, dbeta and the params table fp32 [sc | B | D |
// shift] -- from the producer's sums, or from its own reduce sweep without them. bn_bwd_apply: dx from that table, the
// bits bn_bwd writes.
// mask None: a non-residual BatchNorm + ReLU, the ReLU decision recomputed from x (relu_x) in both halves -- for a
// consumer of dx that forms it on load from dy, x and the table (conv1_fused).
Tensor bn_bwd_params(Tensor dy, Tensor x, OptTensor mask, OptTensor sums, Tensor mean, Tensor invstd, Tensor gamma,
                     Tensor beta, Tensor dgamma, Tensor dbeta) {
  const int C = bn_channels(x, "x");
  const long M = x.numel() / C;
  check_same_shape(dy, x, "dy");
  const bool has_mask = mask && mask->defined();
  const uint8_t* mk = has_mask ? check_bit_mask(*mask, x.numel(), "mask") : nullptr;
  BwdSide a = bwd_side(x, mean, invstd, gamma, beta, dgamma, dbeta, opt_ptr(sums), "sums", M, C);
  launch_bn_bwd_params(cbf(dy), mk, !has_mask, a.nrep, a.s, nullptr, M, C, cur_stream());
  return a.params;
}
Tensor bn_bwd_apply(Tensor dy, Tensor x, OptTensor mask, Tensor params) {
  const int C = bn_channels(x, "x");
  check_same_shape(dy, x, "dy");
  const bool has_mask = mask && mask->defined();
  const uint8_t* mk = has_mask ? check_bit_mask(*mask, x.numel(), "mask") : nullptr;
  check_channel_f32(params, 4L * C, "params");
  TORCH_CHECK(params.device() == x.device(), "params: on x's device");
  auto dx = torch::empty_like(x);
  k8s_amd::BnBwdSide a;
  a.x = cbf(x);
  a.params = f32(params);
  a.dx = bf(dx);
  launch_bn_bwd_apply(cbf(dy), mk, !has_mask, a, nullptr, nullptr, x.numel() / C, C, cur_stream());
  return dx;
}

// Backward of bn_fwd_from_sums_dual: both BatchNorms' dgamma / dbeta and params tables from one masked dy (dy and the
// packed ReLU mask read once per pass). sums / sums2 (optional, together): the reduction done by dy's producer, sums
// (sum g, sum g (x - mean)) and sums2 (slot 1: sum g (x2 - mean2)); without them the dual reduce sweep runs here.
// want_dx: also the apply pass, (dx, dx2); else (params, params2), each [sc | B | D | shift], for
// bn_bwd_apply(dy, x or x2, mask, ...) -- the same bits -- or a consumer that applies a table on load (bwd1x1_fused).
std::vector<Tensor> bn_bwd_dual_impl(bool want_dx, const Tensor& dy, const Tensor& mask, const Tensor& x,
                                     const Tensor& mean, const Tensor& invstd, const Tensor& gamma, const Tensor& beta,
                                     const Tensor& dgamma, const Tensor& dbeta, const Tensor& x2, const Tensor& mean2,
                                     const Tensor& invstd2, const Tensor& gamma2, const Tensor& beta2,
                                     const Tensor& dgamma2, const Tensor& dbeta2, const OptTensor& sums,
                                     const OptTensor& sums2) {
  const Tensor *pre = opt_ptr(sums), *pre2 = opt_ptr(sums2);
  TORCH_CHECK(!pre == !pre2, "sums and sums2 come together");
  const int C = bn_channels(x, "x");
  const long M = x.numel() / C;
  check_same_shape(dy, x, "dy");
  check_same_shape(x2, x, "x2");
  const uint8_t* mk = check_bit_mask(mask, x.numel(), "mask");
  BwdSide a = bwd_side(x, mean, invstd, gamma, beta, dgamma, dbeta, pre, "sums", M, C);
  BwdSide b = bwd_side(x2, mean2, invstd2, gamma2, beta2, dgamma2, dbeta2, pre2, "sums2", M, C);
  TORCH_CHECK(a.nrep == b.nrep, "sums / sums2: the same replica count");
  launch_bn_bwd_params(cbf(dy), mk, false, a.nrep, a.s, &b.s, M, C, cur_stream());
  if (!want_dx) return {a.params, b.params};
  auto dx = torch::empty_like(x), dx2 = torch::empty_like(x);
  a.s.dx = bf(dx);
  b.s.dx = bf(dx2);
  launch_bn_bwd_apply(cbf(dy), mk, false, a.s, &b.s, nullptr, M, C, cur_stream());
  return {dx, dx2};
}
std::vector<Tensor> bn_bwd_dual(Tensor dy, Tensor mask, Tensor x, Tensor mean, Tensor invstd, Tensor gamma,
                                Tensor beta, Tensor dgamma, Tensor dbeta, Tensor x2, Tensor mean2, Tensor invstd2,
                                Tensor gamma2, Tensor beta2, Tensor dgamma2, Tensor dbeta2, OptTensor sums,
                                OptTensor sums2) {
  return bn_bwd_dual_impl(true, dy, mask, x, mean, invstd, gamma, beta, dgamma, dbeta, x2, mean2, invstd2, gamma2,
                          beta2, dgamma2, dbeta2, sums, sums2);
}
std::vector<Tensor> bn_bwd_dual_params(Tensor dy, Tensor mask, Tensor x, Tensor mean, Tensor invstd, Tensor gamma,
                                       Tensor beta, Tensor dgamma, Tensor dbeta, Tensor x2, Tensor mean2,
                                       Tensor invstd2, Tensor gamma2, Tensor beta2, Tensor dgamma2, Tensor dbeta2,
                                       OptTensor sums, OptTensor sums2) {
  return bn_bwd_dual_impl(false, dy, mask, x, mean, invstd, gamma, beta, dgamma, dbeta, x2, mean2, invstd2, gamma2,
                          beta2, dgamma2, dbeta2, sums, sums2);
}

}  // namespace

void bind_batchnorm(pybind11::module_& m) {
  m.def("bn_fwd", &bn_fwd, "x"_a, "res"_a, "gamma"_a, "beta"_a, "run_mean"_a, "run_var"_a, "training"_a, "momentum"_a,
        "eps"_a, "relu"_a, "want_mask"_a = false);
  m.def("bn_bwd", &bn_bwd, "dy"_a, "x"_a, "y"_a, "mean"_a, "invstd"_a, "gamma"_a, "beta"_a, "relu_x"_a, "dgamma"_a,
        "dbeta"_a, "want_dres"_a, "mask"_a = py::none(), "sums"_a = py::none());
  m.def("bn_fwd_from_sums", &bn_fwd_from_sums, "x"_a, "res"_a, "gamma"_a, "beta"_a, "sums"_a, "run_mean"_a, "run_var"_a,
        "momentum"_a, "eps"_a, "relu"_a, "want_mask"_a = false, "want_sub2"_a = false);
  m.def("bn_fwd_from_sums_dual", &bn_fwd_from_sums_dual, "relu(BN(x) + BN_r(xr)), statistics from conv sums");
  m.def("bn_finalize", &bn_finalize, "sums"_a, "gamma"_a, "beta"_a, "run_mean"_a, "run_var"_a, "count"_a, "momentum"_a,
        "eps"_a);
  m.def("bn_bwd_params", &bn_bwd_params, "dy"_a, "x"_a, "mask"_a, "sums"_a, "mean"_a, "invstd"_a, "gamma"_a, "beta"_a,
        "dgamma"_a, "dbeta"_a, "first half of a BatchNorm backward (packed mask, or None: relu_x): dgamma, dbeta, params [sc | B | D | shift]");
  m.def("bn_bwd_apply", &bn_bwd_apply, "dy"_a, "x"_a, "mask"_a, "params"_a,
        "second half of a BatchNorm backward (packed mask, or None: relu_x): dx from bn_bwd_params' table");
  auto def_dual = [&m](const char* name, auto fn, const char* doc) {
    m.def(name, fn, "dy"_a, "mask"_a, "x"_a, "mean"_a, "invstd"_a, "gamma"_a, "beta"_a, "dgamma"_a, "dbeta"_a, "x2"_a,
          "mean2"_a, "invstd2"_a, "gamma2"_a, "beta2"_a, "dgamma2"_a, "dbeta2"_a, "sums"_a = py::none(),
          "sums2"_a = py::none(), doc);
  };
  def_dual("bn_bwd_dual", &bn_bwd_dual,
           "both BatchNorm backwards of bn_fwd_from_sums_dual from one masked dy: (dx, dx2)");
  def_dual("bn_bwd_dual_params", &bn_bwd_dual_params,
           "first half of bn_bwd_dual: both dgamma / dbeta and (params, params2), each [sc | B | D | shift]");
  m.def("bn_relu_maxpool", &bn_relu_maxpool, "x"_a, "sums"_a, "gamma"_a, "beta"_a, "run_mean"_a, "run_var"_a,
        "momentum"_a, "eps"_a, "want_link"_a = false);
  m.def("pool_bn_bwd", &pool_bn_bwd, "dpool"_a, "idx"_a, "x"_a, "mean"_a, "invstd"_a, "gamma"_a, "beta"_a, "dgamma"_a,
        "dbeta"_a, "sums"_a = py::none());
}

}  // namespace k8s_amd::binding
