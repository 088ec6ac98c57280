// Convolution (NHWC x, KRSC w): forward, inference with a folded BatchNorm, the data gradients' parity sub-grid
// products and weight transforms, the 3x3 staged-window data gradient with BatchNorm-backward sums, weight gradients.
#include "binding/common.h"

namespace k8s_amd::binding {
namespace {

int conv_out(int in, int k, int st, int pad, int dil) { return (in + 2 * pad - dil * (k - 1) - 1) / st + 1; }

struct ConvGeom {
  int N, H, W, C, K, R, S;
};
// x [N, H, W, C] against a weight-shaped [K, R, S, C] tensor (w, or a weight gradient); C % 8 == 0 and K % 8 == 0
ConvGeom conv_geom(const Tensor& x, const Tensor& w) {
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4, "x [N,H,W,C], w [K,R,S,C]");
  ConvGeom g{(int)x.size(0), (int)x.size(1), (int)x.size(2), (int)x.size(3),
             (int)w.size(0), (int)w.size(1), (int)w.size(2)};
  TORCH_CHECK(w.size(3) == g.C, "channel mismatch");
  TORCH_CHECK(g.C % 8 == 0 && g.K % 8 == 0, "implicit-GEMM conv needs C % 8 == 0 and K % 8 == 0");
  return g;
}
Tensor conv_fwd(Tensor x, Tensor w, int64_t stride, int64_t pad, int64_t dil, bool out_f32, OptTensor bias, int64_t act,
                OptTensor stats, OptTensor xform) {
  check_bf16(x, "x"); check_bf16(w, "w");
  const auto [N, H, W, C, K, R, S] = conv_geom(x, w);
  TORCH_CHECK(stride >= 1 && dil >= 1, "conv_fwd: stride >= 1, dilation >= 1");
  const int Ho = conv_out(H, R, stride, pad, dil), Wo = conv_out(W, S, stride, pad, dil);
  if (bias) check_channel_f32(*bias, K, "bias");
  if (stats) check_stat_sums(*stats, K, "stats", true);
  const float* xf = xform_ptr(xform, C);
  if (xf) TORCH_CHECK(C % 64 == 0 && !out_f32 && !bias && act == 0,
                      "normalize-on-load convolution: C % 64 == 0, bf16 output, no bias / activation");
  auto y = torch::empty({N, Ho, Wo, K}, x.options().dtype(out_f32 ? at::kFloat : at::kBFloat16));
  launch_conv_fwd(cbf(x), cbf(w), y.data_ptr(), out_f32, N, H, W, C, K, R, S, (int)stride, (int)pad, (int)dil, Ho, Wo,
                  optf(bias), (int)act, 0, stats ? f32(*stats) : nullptr, cur_stream(), nullptr, xf);
  return y;
}

// Inference convolution with the following BatchNorm folded into the epilogue (gemm.hip TileEpi::LeanInfer):
//   y = act(bf16(conv(x, w) * scale + shift) + res); scale / shift fp32 [K], res bf16 [N, Ho, Wo, K] or None.
// Always the tile kernel; a shape outside its contract raises. `out`: write into this bf16 [N, Ho, Wo, K] tensor.
Tensor conv_infer(Tensor x, Tensor w, int64_t stride, int64_t pad, Tensor scale, Tensor shift, OptTensor res,
                  bool relu, OptTensor out) {
  check_bf16_dense(x, 4, "x"); check_bf16_dense(w, 4, "w");
  const auto [N, H, W, C, K, R, S] = conv_geom(x, w);
  TORCH_CHECK(stride >= 1 && pad >= 0, "conv_infer: stride >= 1, pad >= 0");
  check_channel_f32(scale, K, "scale"); check_channel_f32(shift, K, "shift");
  TORCH_CHECK(H + 2 * pad >= R && W + 2 * pad >= S, "conv_infer: the filter does not fit the padded image");
  const int Ho = conv_out(H, R, stride, pad, 1), Wo = conv_out(W, S, stride, pad, 1);
  TORCH_CHECK((long)N * Ho * Wo < (1L << 31), "conv_infer: fewer than 2^31 output pixels");
  const std::vector<int64_t> oshape{N, Ho, Wo, K};
  if (out) {
    check_bf16_dense(*out, 4, "out");
    TORCH_CHECK(out->sizes().vec() == oshape, "out must be [N, Ho, Wo, K]");
  }
  if (res) {
    check_bf16_dense(*res, 4, "res");
    TORCH_CHECK(res->sizes().vec() == oshape, "res must have the output's shape [N, Ho, Wo, K]");
  }
  Tensor y = out ? *out : torch::empty(oshape, x.options());
  launch_conv_infer(cbf(x), cbf(w), bf(y), N, H, W, C, K, R, S, (int)stride, (int)pad, Ho, Wo, f32(scale), f32(shift),
                    res ? cbf(*res) : nullptr, relu, cur_stream());
  return y;
}

// out[n, i*stride + a, j*stride + b, :] (+)= conv(x, w, stride 1, pad)[n, i, j, :] over an Hs x Ws grid (i < Hs,
// j < Ws): one output parity of a stride-s data gradient. x is dy, w [C, Tr, Ts, K] holds the taps of that parity
// (ops/conv.py _dgrad_strided_hip builds it) and out is the full bf16 dx [N, H, W, C]; `accumulate` adds onto out in
// the epilogue (out already holds the residual branch's gradient).
void conv_fwd_subgrid(Tensor x, Tensor w, int64_t pad, int64_t Hs, int64_t Ws, Tensor out, int64_t stride, int64_t a,
                      int64_t b, bool accumulate, OptTensor bn_x, OptTensor bn_mask, OptTensor bn_mean,
                      OptTensor bn_sums, OptTensor bn_gamma, OptTensor bn_beta, OptTensor bn_invstd) {
  check_bf16(x, "x"); check_bf16(w, "w"); check_bf16(out, "out");
  const auto [N, H, W, C, K, R, S] = conv_geom(x, w);
  TORCH_CHECK(out.dim() == 4 && out.size(0) == N && out.size(3) == K, "out shape");
  const int OH = out.size(1), OW = out.size(2);
  TORCH_CHECK(stride >= 1 && a >= 0 && a < stride && b >= 0 && b < stride, "parity out of range");
  TORCH_CHECK(Hs >= 1 && Ws >= 1 && (Hs - 1) * stride + a < OH && (Ws - 1) * stride + b < OW,
              "sub-grid exceeds the output image");
  k8s_amd::SubGrid sg{OH, OW, (int)stride, (int)a, (int)b};
  // bn_*: a BatchNorm's backward sums over `out` (gemm.hip TileEpi::LeanBnBwd, sub-grid rows). mask kind (bn_mask, accumulate): the
  // correction of a residual BatchNorm's sums for the elements this accumulating product changes (the first data
  // gradient into `out` took the sums over its values). relu kind (bn_gamma / bn_beta / bn_invstd, a plain store):
  // the sums of a BatchNorm + ReLU over this parity's stored pixels (the parities partition the output).
  k8s_amd::BnBwdSums bb;
  if (bn_sums) {
    TORCH_CHECK(bn_x && bn_mean, "bn sums: bn_x and bn_mean");
    TORCH_CHECK(bn_mask ? accumulate : !accumulate,
                "bn sums: bn_mask + accumulate (a correction) or bn_gamma / bn_beta / bn_invstd + a plain store");
    TORCH_CHECK(bn_x->sizes() == out.sizes(), "bn_x: the shape of out");
    bb = bn_bwd_sums(*bn_x, *bn_mean, *bn_sums, bn_mask, bn_gamma, bn_beta, bn_invstd, {}, {}, {});
  }
  launch_conv_fwd(cbf(x), cbf(w), out.data_ptr(), false, N, H, W, C, K, R, S, 1, (int)pad, 1, (int)Hs, (int)Ws, nullptr,
                  0, accumulate ? 1 : 0, nullptr, cur_stream(), &sg, nullptr, bn_sums ? &bb : nullptr);
}

// 3x3 / stride-1 / pad-1 data gradient dx = conv(gy, wt) on the staged-window kernel (wt = conv_dgrad_wtrans(w))
// that also accumulates the BatchNorm-backward sums of dx for the non-residual BatchNorm + ReLU relu(BN(x)) that
// produced the convolution's input (conv3x3.hip epilogue): sums[r][0][c] += sum g, sums[r][1][c] += sum g (x - mean),
// g = relu_on(x) ? dx : 0. sums: zeroed fp32 [conv_stat_replicas, 2, C].
Tensor conv3x3_dgrad_bnstats(Tensor gy, Tensor wt, Tensor x, Tensor gamma, Tensor beta, Tensor mean, Tensor invstd,
                             Tensor sums) {
  check_bf16_dense(gy, 4, "gy"); check_bf16_dense(wt, 4, "wt"); check_bf16_dense(x, 4, "x");
  const int N = (int)gy.size(0), H = (int)gy.size(1), W = (int)gy.size(2), Kc = (int)gy.size(3);
  const int C = (int)wt.size(0);
  TORCH_CHECK(wt.size(1) == 3 && wt.size(2) == 3 && wt.size(3) == Kc, "wt: [C, 3, 3, K]");
  TORCH_CHECK(x.size(0) == N && x.size(1) == H && x.size(2) == W && x.size(3) == C, "x: the shape of dx");
  TORCH_CHECK(k8s_amd::conv3x3_eligible(H, W, Kc, C, 3, 3, 1, 1, 1), "conv3x3_dgrad_bnstats: outside the kernel");
  const k8s_amd::BnBwdSums bb = bn_bwd_sums(x, mean, sums, {}, gamma, beta, invstd, {}, {}, {});
  Tensor dx = torch::empty({N, H, W, C}, gy.options());
  launch_conv3x3(cbf(gy), cbf(wt), bf(dx), nullptr, nullptr, N, H, W, Kc, C, cur_stream(), &bb);
  return dx;
}

// A 3x3 / pad-1 convolution (stride 1 or 2) on the 4-wave GEMM with gathered A rows (gemm256.hip ConvGather), always:
// a shape outside conv3x3_w4_ok raises (ops/conv.py asks conv3x3_w4_use, the policy, first). y = conv(x, w), w
// [K, 3, 3, C]; with `stats` (zeroed fp32 [conv_stat_replicas, 2, K]) also the BatchNorm statistics of the stored y.
Tensor conv3x3_w4(const Tensor& x, const Tensor& w, int64_t stride, float* stats, const uint16_t* bn_x,
                  const float* bn_tab, float* bn_sums) {
  check_bf16_dense(x, 4, "x"); check_bf16_dense(w, 4, "w");
  const auto [N, H, W, C, K, R, S] = conv_geom(x, w);
  TORCH_CHECK(R == 3 && S == 3 && k8s_amd::conv3x3_w4_ok(N, H, W, C, K, (int)stride),
              "conv3x3_w4: 3x3, stride 1 or 2, C % 64 == 0, K % 256 == 0, N Ho Wo % 256 == 0, x below 2^31 elements");
  const int Ho = conv_out(H, 3, stride, 1, 1), Wo = conv_out(W, 3, stride, 1, 1);
  Tensor y = torch::empty({N, Ho, Wo, K}, x.options());
  const SkScratch sk(k8s_amd::conv3x3_w4_plan(N, H, W, C, K, (int)stride), x);
  launch_conv3x3_w4(cbf(x), cbf(w), bf(y), N, H, W, C, K, (int)stride, stats, bn_x, bn_tab, bn_sums, sk.slab_ptr(),
                    sk.sync_ptr(), cur_stream());
  return y;
}
Tensor conv3x3_w4_fwd(Tensor x, Tensor w, int64_t stride, OptTensor stats) {
  if (stats) {
    check_stat_sums(*stats, w.size(0), "stats", true);
    TORCH_CHECK(stats->device() == x.device(), "stats: on x's device");
  }
  return conv3x3_w4(x, w, stride, stats ? f32(*stats) : nullptr, nullptr, nullptr, nullptr);
}
// The stride-1 data gradient dx = conv(gy, wt) the same way (wt = conv_dgrad_wtrans(w), [C, 3, 3, K]); with x, gamma,
// beta, mean, invstd and sums (together) also the BatchNorm-backward sums of dx for the relu(BN(x)) that produced the
// convolution's input, as conv3x3_dgrad_bnstats takes them. sums: zeroed fp32 [conv_stat_replicas, 2, C].
Tensor conv3x3_w4_dgrad(Tensor gy, Tensor wt, OptTensor x, OptTensor gamma, OptTensor beta, OptTensor mean,
                        OptTensor invstd, OptTensor sums) {
  if (!sums) {
    TORCH_CHECK(!x && !gamma && !beta && !mean && !invstd, "conv3x3_w4_dgrad: x, gamma, beta, mean, invstd come with sums");
    return conv3x3_w4(gy, wt, 1, nullptr, nullptr, nullptr, nullptr);
  }
  TORCH_CHECK(x && gamma && beta && mean && invstd, "conv3x3_w4_dgrad: sums need x, gamma, beta, mean and invstd");
  TORCH_CHECK(gy.dim() == 4 && wt.dim() == 4 && x->dim() == 4 && x->size(0) == gy.size(0) && x->size(1) == gy.size(1) &&
                  x->size(2) == gy.size(2) && x->size(3) == wt.size(0),
              "x: the shape of dx");
  bn_bwd_sums(*x, *mean, *sums, {}, gamma, beta, invstd, {}, {}, {});  // (the checks of the relu kind)
  TORCH_CHECK(x->device() == gy.device() && sums->device() == gy.device(), "x and sums: on gy's device");
  Tensor tab = torch::cat({*gamma, *beta, *mean, *invstd});
  return conv3x3_w4(gy, wt, 1, nullptr, cbf(*x), f32(tab), f32(*sums));
}

// The fused backward of a 1x1 / stride-1 convolution whose input is relu(BN(x)) normalised on load (bwd1x1_fused.hip):
// returns dz [M, C] = gy [M, K] . w [K, C]; writes (accumulate: adds) dw [K, C] fp32 = gy^T . relu(bf16(x scale +
// shift)) with xform = fp32 [2, C] (scale | shift), and adds the BatchNorm-backward sums of dz (g = relu_on(x) ? dz : 0:
// sum g, sum g (x - mean)) into sums, zeroed fp32 [conv_stat_replicas, 2, C].
// x3, mask, params (optional, together): gy is the incoming dy of the residual BatchNorm that produced the convolution's
// output, whose backward the kernel applies as it loads -- gy's tiles become bf16(fma(sc, mask ? dy : 0, fma(B, x3, D)))
// with x3 bf16 [M, K], mask the packed ReLU bits uint8 [M, K / 8] and params fp32 [sc | B | D] (3K or more).
// addend, winner_x, winner_bits, winner_mean (optional, together, (C, K) = (64, 256), and then without xform / gamma /
// beta / mean / invstd): the final form, for a convolution reading a stored x whose data gradient is the second into
// it. dw = gy^T . x with x as stored; the result bf16(bf16(gy . w) + addend) (the tile kernel's accumulating epilogue's
// rounding) is written over addend [M, C] and addend itself is returned; sums take the pool kind's g = bit ? stored result : 0, sum g and sum g (winner_x -
// winner_mean), winner_x bf16 [M, C] and winner_bits uint8 [M * C / 8] from the pooled forward (bn_relu_maxpool).
Tensor bwd1x1_fused(Tensor gy, Tensor x, Tensor w, OptTensor xform, OptTensor gamma, OptTensor beta, OptTensor mean,
                    OptTensor invstd, Tensor dw, Tensor sums, bool accumulate, OptTensor x3, OptTensor mask,
                    OptTensor params, OptTensor addend, OptTensor winner_x, OptTensor winner_bits,
                    OptTensor winner_mean) {
  check_bf16_dense(gy, 2, "gy"); check_bf16_dense(x, 2, "x"); check_bf16_dense(w, 2, "w");
  const long M = gy.size(0), K = gy.size(1), C = x.size(1);
  TORCH_CHECK(x.size(0) == M && w.size(0) == K && w.size(1) == C, "shapes: gy [M, K], x [M, C], w [K, C]");
  TORCH_CHECK(k8s_amd::bwd1x1_fused_ok(M, (int)C, (int)K),
              "bwd1x1_fused: (C, K) = (64, 256) or (128, 512), 1 <= M < 2^31");
  check_cuda(dw, "dw"); check_dtype(dw, at::kFloat, "dw"); check_aligned(dw, "dw");
  TORCH_CHECK(dw.numel() == K * C, "dw must have K * C fp32 elements");
  const bool fin = addend || winner_x || winner_bits || winner_mean;
  k8s_amd::BnBwdSums bb;
  k8s_amd::Bwd1x1Final fn;
  if (fin) {
    TORCH_CHECK(addend && winner_x && winner_bits && winner_mean,
                "bwd1x1_fused: addend, winner_x, winner_bits and winner_mean come together");
    TORCH_CHECK(!xform && !gamma && !beta && !mean && !invstd,
                "bwd1x1_fused: the final form takes x as stored -- no xform, gamma, beta, mean or invstd");
    TORCH_CHECK(k8s_amd::bwd1x1_final_ok(M, (int)C, (int)K), "bwd1x1_fused: the final form is (C, K) = (64, 256) only");
    check_bf16_dense(*addend, 2, "addend"); check_bf16_dense(*winner_x, 2, "winner_x");
    TORCH_CHECK(addend->size(0) == M && addend->size(1) == C, "addend: the shape of x, [M, C]");
    TORCH_CHECK(winner_x->size(0) == M && winner_x->size(1) == C, "winner_x: the shape of x, [M, C]");
    fn.winner_bits = check_bit_mask(*winner_bits, M * C, "winner_bits");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(fn.winner_bits) & 3) == 0, "winner_bits must be 4-byte aligned");
    check_channel_f32(*winner_mean, C, "winner_mean");
    check_stat_sums(sums, C, "bn sums", true);
    TORCH_CHECK(addend->device() == gy.device() && winner_x->device() == gy.device() &&
                    winner_bits->device() == gy.device() && winner_mean->device() == gy.device() &&
                    sums.device() == gy.device(),
                "addend, winner_x, winner_bits, winner_mean and sums: on gy's device");
    fn.addend = cbf(*addend);
    fn.winner_x = cbf(*winner_x);
    fn.winner_mean = f32(*winner_mean);
    bb.sums = f32(sums);
  } else {
    TORCH_CHECK(xform && gamma && beta && mean && invstd, "bwd1x1_fused: xform, gamma, beta, mean and invstd");
    check_channel_f32(*xform, 2 * C, "xform (BatchNorm scale | shift)");
    bb = bn_bwd_sums(x, *mean, sums, {}, gamma, beta, invstd, {}, {}, {});
  }
  k8s_amd::Bwd1x1Bn3 bn3;
  const bool onload = x3 || mask || params;
  if (onload) {
    TORCH_CHECK(x3 && mask && params, "bwd1x1_fused: x3, mask and params come together");
    check_bf16_dense(*x3, 2, "x3");
    TORCH_CHECK(x3->size(0) == M && x3->size(1) == K, "x3: the shape of gy, [M, K]");
    bn3.mask = check_bit_mask(*mask, M * K, "mask");
    check_aligned(*mask, "mask");
    check_cuda(*params, "params"); check_dtype(*params, at::kFloat, "params"); check_aligned(*params, "params");
    TORCH_CHECK(params->numel() >= 3 * K, "params: fp32 [sc | B | D], 3K elements or more");
    TORCH_CHECK(x3->device() == gy.device() && mask->device() == gy.device() && params->device() == gy.device(),
                "x3, mask and params: on gy's device");
    bn3.x3 = cbf(*x3);
    bn3.params = f32(*params);
  }
  Tensor dz = fin ? *addend : torch::empty({M, C}, gy.options());
  Tensor part;  // the final form's per-workgroup dW slabs
  if (fin) {
    part = torch::empty({k8s_amd::bwd1x1_final_workspace(M, (int)C, (int)K)}, dw.options());
    fn.dw_partials = f32(part);
  }
  launch_bwd1x1_fused(cbf(gy), cbf(x), cbf(w), fin ? nullptr : f32(*xform), bb.gamma, bb.beta, bb.mean, bb.invstd,
                      bf(dz), f32(dw), bb.sums, M, (int)C, (int)K, accumulate, cur_stream(), onload ? &bn3 : nullptr,
                      fin ? &fn : nullptr);
  return dz;
}

// The fused backward of the 1x1 / stride-1 convolution that opens a ResNet identity bottleneck, with the apply pass of
// the BatchNorm + ReLU behind it formed on load (conv1_fused.hip). dz1 / x1 [M, W]: that BatchNorm's incoming gradient
// and input, params its fp32 [sc | B | D | shift] table (bn_bwd_params with mask None); w [W, N]; xin [M, N] the
// convolution's input. Returns dx [M, N] = bf16(bf16(dx1 . w) + (add_mask ? add_src : 0)) with dx1 =
// bf16(fma(sc, relu_on(x1) ? dz1 : 0, fma(B, x1, D))) never stored; writes (accumulate: adds) dw [W, N] fp32 =
// dx1^T . xin; adds the BatchNorm-backward sums of dx (g = mask ? dx : 0: sum g, sum g (x - mean)) into sums, zeroed
// fp32 [conv_stat_replicas, 2, N]. (W, N) = (64, 256) or (128, 512).
Tensor conv1_fused(Tensor dz1, Tensor x1, Tensor params, Tensor w, Tensor xin, Tensor add_src, Tensor add_mask,
                   Tensor x, Tensor mask, Tensor mean, Tensor sums, Tensor dw, bool accumulate) {
  check_bf16_dense(dz1, 2, "dz1"); check_bf16_dense(x1, 2, "x1"); check_bf16_dense(w, 2, "w");
  check_bf16_dense(xin, 2, "xin"); check_bf16_dense(add_src, 2, "add_src"); check_bf16_dense(x, 2, "x");
  for (const Tensor* t : {&dz1, &x1, &w, &xin, &add_src, &x, &add_mask, &mask, &params, &mean, &sums, &dw})
    check_cuda(*t, "conv1_fused operand");
  const long M = dz1.size(0), W = dz1.size(1), N = w.size(1);
  TORCH_CHECK(k8s_amd::conv1_fused_ok(M, (int)W, (int)N), "conv1_fused: (W, N) = (64, 256) or (128, 512), 1 <= M < 2^31");
  TORCH_CHECK(x1.sizes() == dz1.sizes() && w.size(0) == W && xin.size(0) == M && xin.size(1) == N &&
                  add_src.sizes() == xin.sizes() && x.sizes() == xin.sizes(),
              "shapes: dz1 / x1 [M, W], w [W, N], xin / add_src / x [M, N]");
  k8s_amd::Conv1Fused c;
  c.abits = check_bit_mask(add_mask, M * N, "add_mask"); check_aligned(add_mask, "add_mask");
  c.bits = check_bit_mask(mask, M * N, "mask"); check_aligned(mask, "mask");
  check_channel_f32(params, 4 * W, "params"); check_aligned(params, "params");
  check_channel_f32(mean, N, "mean");
  check_stat_sums(sums, N, "sums", true);
  check_cuda(dw, "dw"); check_dtype(dw, at::kFloat, "dw"); check_aligned(dw, "dw");
  TORCH_CHECK(dw.numel() == W * N, "dw must have W * N fp32 elements");
  for (const Tensor* t : {&x1, &w, &xin, &add_src, &x, &add_mask, &mask, &params, &mean, &sums, &dw})
    TORCH_CHECK(t->device() == dz1.device(), "conv1_fused: every operand on dz1's device");
  Tensor dx = torch::empty({M, N}, dz1.options());
  Tensor part = torch::empty({k8s_amd::conv1_fused_workspace(M, (int)W, (int)N)}, dw.options());
  c.dz1 = cbf(dz1); c.x1 = cbf(x1); c.params = f32(params); c.w = cbf(w); c.xin = cbf(xin); c.dy = cbf(add_src);
  c.x3 = cbf(x); c.mean = f32(mean); c.dx = bf(dx); c.sums = f32(sums); c.dw = f32(dw); c.dw_partials = f32(part);
  launch_conv1_fused(c, M, (int)W, (int)N, accumulate, cur_stream());
  return dx;
}

// The 3x3 / pad-1 weight gradient dw [K, 3, 3, C] fp32 (+)= dy^T . im2col(x) on the 4-wave GEMM with gathered B rows
// (gemm256.hip), always: a shape outside conv3x3_w4_wgrad_ok raises (conv_wgrad asks conv3x3_w4_wgrad_use first).
void conv3x3_w4_wgrad(Tensor x, Tensor dy, Tensor dw, int64_t stride, bool accumulate) {
  check_bf16_dense(x, 4, "x"); check_bf16_dense(dy, 4, "dy");
  check_cuda(dw, "dw"); check_dtype(dw, at::kFloat, "dw"); check_aligned(dw, "dw");
  const auto [N, H, W, C, K, R, S] = conv_geom(x, dw);
  TORCH_CHECK(R == 3 && S == 3 && k8s_amd::conv3x3_w4_wgrad_ok(N, H, W, C, K, (int)stride),
              "conv3x3_w4_wgrad: 3x3, stride 1 or 2, C % 256 == 0, K % 256 == 0, N Ho Wo % 64 == 0");
  TORCH_CHECK(dy.size(0) == N && dy.size(1) == conv_out(H, 3, stride, 1, 1) && dy.size(2) == conv_out(W, 3, stride, 1, 1) &&
                  dy.size(3) == K && dy.device() == x.device() && dw.device() == x.device(),
              "dy shape / device mismatch");
  Tensor ws;
  const long nws = k8s_amd::conv3x3_w4_wgrad_workspace(N, H, W, C, K, (int)stride);
  if (nws) ws = torch::empty({nws}, dw.options());
  launch_conv3x3_w4_wgrad(cbf(x), cbf(dy), f32(dw), N, H, W, C, K, (int)stride, accumulate, nws ? f32(ws) : nullptr,
                          cur_stream());
}

// dw[K,R,S,C] fp32 (+)= dy^T . im2col(x)
void conv_wgrad(Tensor x, Tensor dy, Tensor dw, int64_t stride, int64_t pad, int64_t dil, int64_t splits,
                bool accumulate, OptTensor xform) {
  check_bf16(x, "x"); check_bf16(dy, "dy");
  check_cuda(dw, "dw"); check_dtype(dw, at::kFloat, "dw");
  const auto [N, H, W, C, K, R, S] = conv_geom(x, dw);
  TORCH_CHECK(stride >= 1 && dil >= 1, "conv_wgrad: stride >= 1, dilation >= 1");
  const int Ho = conv_out(H, R, stride, pad, dil), Wo = conv_out(W, S, stride, pad, dil);
  TORCH_CHECK(dy.dim() == 4 && dy.size(0) == N && dy.size(1) == Ho && dy.size(2) == Wo && dy.size(3) == K,
              "dy shape mismatch");
  const float* xf = xform_ptr(xform, C);
  // the 256 / 512-channel 3x3 layers on a chip-filling grid: the 4-wave GEMM with gathered B rows (gemm256.hip)
  if (!xf && splits <= 0 && R == 3 && S == 3 && pad == 1 && dil == 1 &&
      k8s_amd::conv3x3_w4_wgrad_use(N, H, W, C, K, (int)stride)) {
    conv3x3_w4_wgrad(x, dy, dw, stride, accumulate);
    return;
  }
  if (dil == 1 && Ho == H && Wo == W && H == W && k8s_amd::wgrad3x3_tiled_ok(C, K, R, S, (int)stride, (int)pad, W)) {
    auto wsp = torch::empty({k8s_amd::wgrad3x3_tiled_workspace(N, H, W, C)}, dw.options());
    launch_wgrad3x3_tiled(cbf(x), cbf(dy), f32(wsp), f32(dw), N, H, W, C, accumulate, cur_stream(), xf);
    return;
  }
  if (!xf && dil == 1 && k8s_amd::wgrad_stream_eligible(N, Ho, Wo, C, K, R, S)) {
    launch_wgrad_stream(cbf(x), cbf(dy), f32(dw), N, H, W, C, K, R, S, (int)stride, (int)pad, Ho, Wo, accumulate,
                        cur_stream());
    return;
  }
  if (xf) TORCH_CHECK(C % 64 == 0, "normalize-on-load weight gradient needs C % 64 == 0");
  int sp = splits <= 0 ? k8s_amd::gemm_choose_splits(K, R * S * C, N * Ho * Wo) : (int)splits;
  Tensor ws;
  if (sp > 1) ws = torch::empty({k8s_amd::gemm_splitk_workspace(K, R * S * C, sp)}, dw.options());
  launch_conv_wgrad(cbf(x), cbf(dy), f32(dw), N, H, W, C, K, R, S, (int)stride, (int)pad, (int)dil, Ho, Wo, sp,
                    accumulate, sp > 1 ? f32(ws) : nullptr, cur_stream(), xf);
}

// taps: per parity, the list of r*S + s tap indices (row-major over its [Tr][Ts] grid); returns one packed bf16
// buffer with parity p's [C, T_p, K] sub-weight at the element offset offsets[p]
std::vector<Tensor> conv_dgrad_wsub(Tensor w, std::vector<std::vector<int64_t>> taps) {
  check_bf16(w, "w");
  TORCH_CHECK(w.dim() == 4, "w [K,R,S,C]");
  const int K = w.size(0), R = w.size(1), S = w.size(2), C = w.size(3);
  TORCH_CHECK(!taps.empty() && taps.size() <= 16, "1-16 parities");
  k8s_amd::DgradTaps t{};
  long off = 0;
  std::vector<int64_t> offs;
  for (size_t p = 0; p < taps.size(); ++p) {
    TORCH_CHECK(!taps[p].empty() && taps[p].size() <= 16, "1-16 taps per parity");
    t.n[p] = (int)taps[p].size();
    t.off[p] = off;
    offs.push_back(off);
    for (size_t i = 0; i < taps[p].size(); ++i) {
      TORCH_CHECK(taps[p][i] >= 0 && taps[p][i] < R * S, "tap index out of range");
      t.rs[p][i] = (int)taps[p][i];
    }
    off += (long)C * t.n[p] * K;
    off = (off + 7) / 8 * 8;  // keep every parity's sub-weight 16-B aligned
  }
  auto out = torch::empty({off}, w.options());
  launch_conv_dgrad_wsub(cbf(w), bf(out), K, R * S, C, t, (int)taps.size(), cur_stream());
  return {out, torch::tensor(offs)};
}
Tensor conv_dgrad_wtrans(Tensor w) {
  check_bf16(w, "w");
  TORCH_CHECK(w.dim() == 4, "w [K,R,S,C]");
  const int K = w.size(0), R = w.size(1), S = w.size(2), C = w.size(3);
  auto w2 = torch::empty({C, R, S, K}, w.options());
  launch_conv_dgrad_wtrans(cbf(w), bf(w2), K, R, S, C, cur_stream());
  return w2;
}

}  // namespace

void bind_conv(pybind11::module_& m) {
  m.def("conv_fwd", &conv_fwd, "x"_a, "w"_a, "stride"_a, "pad"_a, "dil"_a, "out_f32"_a, "bias"_a, "act"_a, "stats"_a,
        "xform"_a = py::none());
  m.def("conv_infer", &conv_infer, "x"_a, "w"_a, "stride"_a, "pad"_a, "scale"_a, "shift"_a, "res"_a = py::none(),
        "relu"_a = true, "out"_a = py::none());
  m.def("conv3x3_staged_ok", [](int H, int W, int C, int K, int R, int S, int stride, int pad) {
    // the staged-window forward / data gradient (conv3x3.hip) and the tiled weight gradient (wgrad_tile.hip) both
    // take this layer: BatchNorm + ReLU can be normalised on load in all three products
    return k8s_amd::conv3x3_eligible(H, W, C, K, R, S, stride, pad, 1) &&
           k8s_amd::conv3x3_eligible(H, W, K, C, R, S, stride, pad, 1) &&
           k8s_amd::wgrad3x3_tiled_ok(C, K, R, S, stride, pad, W);
  });
  m.def("conv3x3_dgrad_bnstats", &conv3x3_dgrad_bnstats,
        "3x3 stride-1 data gradient with the BatchNorm-backward sums of a relu(BN(x)) input (conv3x3.hip)");
  m.def("conv3x3_w4_fwd", &conv3x3_w4_fwd, "x"_a, "w"_a, "stride"_a, "stats"_a = py::none(),
        "3x3 pad-1 convolution (stride 1 / 2) on the 4-wave GEMM with gathered A rows (gemm256.hip ConvGather)");
  m.def("conv3x3_w4_dgrad", &conv3x3_w4_dgrad, "gy"_a, "wt"_a, "x"_a = py::none(), "gamma"_a = py::none(),
        "beta"_a = py::none(), "mean"_a = py::none(), "invstd"_a = py::none(), "sums"_a = py::none(),
        "3x3 stride-1 data gradient on the same kernel, optionally with the BatchNorm-backward sums of dx");
  m.def("conv3x3_w4_ok", &k8s_amd::conv3x3_w4_ok, "N"_a, "H"_a, "W"_a, "C"_a, "K"_a, "stride"_a,
        "the contract of conv3x3_w4_fwd / _dgrad (a data gradient: C and K exchanged)");
  m.def("conv3x3_w4_use", &k8s_amd::conv3x3_w4_use, "N"_a, "H"_a, "W"_a, "C"_a, "K"_a, "stride"_a, "dgrad"_a,
        "the policy: K8S_AMD_CONV3X3_W4, a chip-filling grid and the shapes where the route measured faster");
  m.def("conv3x3_w4_wgrad", &conv3x3_w4_wgrad, "x"_a, "dy"_a, "dw"_a, "stride"_a, "accumulate"_a,
        "3x3 pad-1 weight gradient (stride 1 / 2) on the 4-wave GEMM with gathered B rows");
  m.def("conv3x3_w4_wgrad_ok", &k8s_amd::conv3x3_w4_wgrad_ok, "N"_a, "H"_a, "W"_a, "C"_a, "K"_a, "stride"_a);
  m.def("conv3x3_w4_wgrad_use", &k8s_amd::conv3x3_w4_wgrad_use, "N"_a, "H"_a, "W"_a, "C"_a, "K"_a, "stride"_a,
        "whether conv_wgrad routes this layer there: K8S_AMD_CONV3X3_W4 and a chip-filling grid");
  m.def("conv3x3_w4_tail_splits", [](int N, int H, int W, int C, int K, int stride) {
    return k8s_amd::conv3x3_w4_plan(N, H, W, C, K, stride).sk;
  }, "K splits of the launch's stream-K tail (1: no tail)");
  m.def("conv_fwd_subgrid", &conv_fwd_subgrid, "x"_a, "w"_a, "pad"_a, "Hs"_a, "Ws"_a, "out"_a, "stride"_a, "a"_a, "b"_a,
        "accumulate"_a = false, "bn_x"_a = py::none(), "bn_mask"_a = py::none(), "bn_mean"_a = py::none(),
        "bn_sums"_a = py::none(), "bn_gamma"_a = py::none(), "bn_beta"_a = py::none(), "bn_invstd"_a = py::none());
  m.def("conv_wgrad", &conv_wgrad, "x"_a, "dy"_a, "dw"_a, "stride"_a, "pad"_a, "dil"_a, "splits"_a, "accumulate"_a,
        "xform"_a = py::none());
  m.def("bwd1x1_fused", &bwd1x1_fused, "gy"_a, "x"_a, "w"_a, "xform"_a, "gamma"_a, "beta"_a, "mean"_a, "invstd"_a,
        "dw"_a, "sums"_a, "accumulate"_a, "x3"_a = py::none(), "mask"_a = py::none(), "params"_a = py::none(),
        "addend"_a = py::none(), "winner_x"_a = py::none(), "winner_bits"_a = py::none(),
        "winner_mean"_a = py::none(),
        "1x1 data gradient, normalize-on-load weight gradient and BatchNorm-backward sums in one pass (bwd1x1_fused.hip)");
  m.def("bwd1x1_fused_ok", [](int64_t M, int64_t C, int64_t K) {
    return C <= 1024 && K <= 4096 && k8s_amd::bwd1x1_fused_ok(M, (int)C, (int)K);
  }, "M"_a, "C"_a, "K"_a, "whether bwd1x1_fused takes this shape");
  m.def("bwd1x1_final_ok", [](int64_t M, int64_t C, int64_t K) {
    return C <= 1024 && K <= 4096 && k8s_amd::bwd1x1_final_ok(M, (int)C, (int)K);
  }, "M"_a, "C"_a, "K"_a, "whether bwd1x1_fused's final form (addend, winner_*) takes this shape");
  m.def("conv1_fused", &conv1_fused, "dz1"_a, "x1"_a, "params"_a, "w"_a, "xin"_a, "add_src"_a, "add_mask"_a, "x"_a,
        "mask"_a, "mean"_a, "sums"_a, "dw"_a, "accumulate"_a,
        "identity-block conv1 backward with bn1's apply pass on load: dx, dw and the sums in one pass (conv1_fused.hip)");
  m.def("conv1_fused_ok", [](int64_t M, int64_t W, int64_t N) {
    return W <= 1024 && N <= 4096 && k8s_amd::conv1_fused_ok(M, (int)W, (int)N);
  }, "M"_a, "W"_a, "N"_a, "whether conv1_fused takes this shape");
  m.def("wgrad_stream_eligible",&k8s_amd::wgrad_stream_eligible, "tall-K weight-gradient kernel takes this shape");
  m.def("conv_dgrad_wtrans", &conv_dgrad_wtrans);
  m.def("conv_dgrad_wsub", &conv_dgrad_wsub);
}

}  // namespace k8s_amd::binding
