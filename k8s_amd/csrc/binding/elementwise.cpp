// Elementwise kernels (SwiGLU, rotary embedding, activation backwards, column sums, packed-mask apply), max / average
// pooling, the embedding gather and the space-to-depth ResNet stem.
#include "binding/common.h"

namespace k8s_amd::binding {
namespace {

Tensor mask_apply(Tensor src, Tensor mask) {
  check_bf16(src, "src");
  const uint8_t* mk = check_bit_mask(mask, src.numel(), "mask");
  Tensor out = torch::empty_like(src);
  launch_mask_apply(cbf(src), mk, bf(out), src.numel(), cur_stream());
  return out;
}
void check_swiglu_blk(long F2, int64_t blk) {
  TORCH_CHECK(blk == 0 || (blk > 0 && blk % 8 == 0 && (F2 / 2) % blk == 0), "swiglu: blk must divide F (multiple of 8)");
}
Tensor swiglu_fwd(Tensor gu, int64_t blk) {
  check_bf16(gu, "gu");
  TORCH_CHECK(gu.dim() >= 1 && gu.size(-1) > 0 && gu.size(-1) % 16 == 0, "2F must be a multiple of 16");
  const long F2 = gu.size(-1);
  const long T = gu.numel() / F2;
  check_swiglu_blk(F2, blk);
  auto sizes = gu.sizes().vec();
  sizes.back() = F2 / 2;
  auto y = torch::empty(sizes, gu.options());
  launch_swiglu_fwd(cbf(gu), bf(y), T, (int)(F2 / 2), (int)blk, cur_stream());
  return y;
}
Tensor swiglu_bwd(Tensor gu, Tensor dy, int64_t blk) {
  check_bf16(gu, "gu"); check_bf16(dy, "dy");
  TORCH_CHECK(gu.dim() >= 1 && gu.size(-1) > 0 && gu.size(-1) % 16 == 0, "2F must be a multiple of 16");
  const long F2 = gu.size(-1);
  TORCH_CHECK(dy.numel() * 2 == gu.numel(), "dy: half of gu");
  check_swiglu_blk(F2, blk);
  auto dgu = torch::empty_like(gu);
  launch_swiglu_bwd(cbf(gu), cbf(dy), bf(dgu), gu.numel() / F2, (int)(F2 / 2), (int)blk, cur_stream());
  return dgu;
}

// in place on x [T, H*D]: contiguous, or a 2-D column slice of a wider row-major tensor (row stride = its
// leading dimension -- the q and k heads of a packed QKV projection rotated without a copy)
void rope_(Tensor x, Tensor pos, Tensor table, bool inverse) {
  TORCH_CHECK(x.is_cuda(), "x must be a GPU tensor"); check_dtype(x, at::kBFloat16, "x");
  check_cuda(pos, "pos"); check_dtype(pos, at::kInt, "pos");
  check_cuda(table, "table"); check_dtype(table, at::kFloat, "table");
  TORCH_CHECK(table.dim() >= 2, "table: [maxpos, D / 2, 2]");
  const int D = (int)table.size(1) * 2;
  TORCH_CHECK(D > 0 && D % 16 == 0, "head dim must be a multiple of 16");
  const long T = pos.numel();
  long ld;
  int H;
  if (x.is_contiguous()) {
    TORCH_CHECK(T > 0 && x.numel() % (T * D) == 0, "x must be [T, H*D]");
    H = (int)(x.numel() / (T * D));
    ld = (long)H * D;
  } else {
    TORCH_CHECK(x.dim() == 2 && x.size(0) == T && x.stride(1) == 1 && x.size(1) % D == 0 && x.stride(0) % 8 == 0,
                "strided x must be a [T, H*D] column slice with unit column stride");
    check_aligned(x, "x");
    H = (int)(x.size(1) / D);
    ld = x.stride(0);
  }
  launch_rope(bf(x), ld, pos.data_ptr<int>(), f32(table), T, H, D, inverse, cur_stream());
}

// dx from dy and the activation's saved tensor (GELU: the pre-activation, ReLU: the output)
template <class Launch>
Tensor act_bwd(const Tensor& dy, const Tensor& saved, Launch launch) {
  check_bf16(dy, "dy"); check_bf16(saved, "pre / y");
  TORCH_CHECK(dy.numel() == saved.numel() && dy.numel() % 8 == 0, "dy / saved: the same multiple of 8 elements");
  auto dx = torch::empty_like(dy);
  launch(cbf(dy), cbf(saved), bf(dx), dy.numel(), cur_stream());
  return dx;
}
Tensor gelu_bwd(Tensor dy, Tensor pre) { return act_bwd(dy, pre, launch_gelu_bwd); }
Tensor relu_bwd(Tensor dy, Tensor y) { return act_bwd(dy, y, launch_relu_bwd); }

// rows of C % 8 == 0 bf16 columns; returns C
int colsum_cols(const Tensor& x, const char* name) {
  check_bf16(x, name);
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0 && x.size(-1) % 8 == 0, name, ": rows of C % 8 == 0 columns");
  return (int)x.size(-1);
}
// `out` (optional, fp32 [C] contiguous, e.g. a bias's flat gradient slot) is written in place instead of a new tensor
Tensor colsum_out(const OptTensor& out, const Tensor& x, int C) {
  if (!out) return torch::empty({C}, x.options().dtype(at::kFloat));
  check_channel_f32(*out, C, "out");
  return *out;
}
// column sums of a [R, C] bf16 matrix in fp32
Tensor colsum(Tensor x, OptTensor out_) {
  const int C = colsum_cols(x, "x");
  const long R = x.numel() / C;
  Tensor out = colsum_out(out_, x, C);
  auto work = torch::empty({k8s_amd::colsum_workspace_floats(R, C)}, out.options());
  launch_colsum(cbf(x), R, C, f32(work), f32(out), false, cur_stream());
  return out;
}

// activation backward + the column sums of its result (a linear's bias gradient); returns [g, db]
std::vector<Tensor> act_bwd_colsum(Tensor dy, Tensor pre, int64_t act, OptTensor out_) {
  const int C = colsum_cols(dy, "dy");
  check_bf16(pre, "pre");
  TORCH_CHECK(act == 1 || act == 2, "act: 1 ReLU, 2 GELU(tanh)");
  TORCH_CHECK(dy.sizes() == pre.sizes(), "dy / pre: the same shape");
  const long R = dy.numel() / C;
  Tensor out = colsum_out(out_, dy, C);
  auto g = torch::empty_like(dy);
  auto work = torch::empty({k8s_amd::colsum_workspace_floats(R, C)}, out.options());
  launch_act_bwd_colsum((int)act, cbf(dy), cbf(pre), bf(g), R, C, f32(work), f32(out), false, cur_stream());
  return {g, out};
}

// ------------------------------------------------------------------ max / average pooling (NHWC)
std::vector<Tensor> maxpool_fwd(Tensor x, int64_t k, int64_t s, int64_t p) {
  check_bf16(x, "x");
  TORCH_CHECK(x.dim() == 4 && x.size(3) % 8 == 0, "x must be NHWC with C % 8 == 0");
  TORCH_CHECK(k >= 1 && k <= 15 && p >= 0 && p < k && s >= 1, "window too large");
  const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int Ho = (H + 2 * p - k) / s + 1, Wo = (W + 2 * p - k) / s + 1;
  auto y = torch::empty({N, Ho, Wo, C}, x.options());
  auto idx = torch::empty({N, Ho, Wo, C}, x.options().dtype(at::kByte));
  launch_maxpool_fwd(cbf(x), bf(y), idx.data_ptr<uint8_t>(), N, H, W, C, Ho, Wo, (int)k, (int)s, (int)p, cur_stream());
  return {y, idx};
}
Tensor maxpool_bwd(Tensor dy, Tensor idx, int64_t H, int64_t W, int64_t k, int64_t s, int64_t p) {
  check_bf16(dy, "dy");
  check_cuda(idx, "idx"); check_dtype(idx, at::kByte, "idx");
  TORCH_CHECK(dy.sizes() == idx.sizes() && dy.dim() == 4 && dy.size(3) % 8 == 0, "dy / idx mismatch");
  TORCH_CHECK(k >= 1 && k <= 15 && p >= 0 && p < k && s >= 1 && H >= 1 && W >= 1, "window too large");
  const int N = dy.size(0), Ho = dy.size(1), Wo = dy.size(2), C = dy.size(3);
  TORCH_CHECK(Ho == (H + 2 * p - k) / s + 1 && Wo == (W + 2 * p - k) / s + 1, "input size mismatch");
  auto dx = torch::empty({N, H, W, C}, dy.options());
  launch_maxpool_bwd(cbf(dy), idx.data_ptr<uint8_t>(), bf(dx), N, (int)H, (int)W, C, Ho, Wo, (int)k, (int)s, (int)p,
                     cur_stream());
  return dx;
}
Tensor avgpool_fwd(Tensor x) {
  check_bf16(x, "x");
  TORCH_CHECK(x.dim() == 4 && x.size(3) % 8 == 0, "x must be NHWC with C % 8 == 0");
  const int N = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
  auto y = torch::empty({N, C}, x.options());
  launch_avgpool_fwd(cbf(x), bf(y), N, HW, C, cur_stream());
  return y;
}
Tensor avgpool_bwd(Tensor dy, int64_t H, int64_t W) {
  check_bf16(dy, "dy");
  TORCH_CHECK(dy.dim() == 2 && dy.size(1) % 8 == 0 && H >= 1 && W >= 1, "dy must be [N, C] with C % 8 == 0");
  const int N = dy.size(0), C = dy.size(1);
  auto dx = torch::empty({N, H, W, C}, dy.options());
  launch_avgpool_bwd(cbf(dy), bf(dx), N, (int)(H * W), C, cur_stream());
  return dx;
}

// ------------------------------------------------------------------ embedding (sum of gathers)
// ids: int64 [T] on the GPU, or None = the position table (row t % S), which needs T % S == 0 and >= S rows
const int64_t* embed_ids(const c10::optional<Tensor>& ids, long T, long S, long rows) {
  if (!ids) {
    TORCH_CHECK(S > 0 && T % S == 0 && rows >= S, "position table needs T % S == 0 and >= S rows");
    return nullptr;
  }
  check_cuda(*ids, "ids"); check_dtype(*ids, at::kLong, "ids");
  TORCH_CHECK(ids->numel() == T, "ids must have T entries");
  return ids->data_ptr<int64_t>();
}

// tables: list of (weight bf16 [V, D], ids int64 [T] or None = position table) ; returns bf16 [T, D]
Tensor embed_fwd(std::vector<Tensor> weights, std::vector<c10::optional<Tensor>> ids, int64_t T, int64_t S) {
  TORCH_CHECK(!weights.empty() && weights.size() <= 3 && weights.size() == ids.size(), "1-3 tables, one ids each");
  TORCH_CHECK(weights[0].dim() == 2 && T >= 0, "tables must be [V, D]");
  const long D = weights[0].size(1);
  k8s_amd::EmbTable tabs[3];
  for (size_t i = 0; i < weights.size(); ++i) {
    const Tensor& w = weights[i];
    check_bf16(w, "weight");
    TORCH_CHECK(w.dim() == 2 && w.size(1) == D && D % 8 == 0, "tables must be [V, D] with one D % 8 == 0");
    tabs[i] = k8s_amd::EmbTable{cbf(w), nullptr, embed_ids(ids[i], T, S, w.size(0)), (int)w.size(0)};
  }
  auto out = torch::empty({T, D}, weights[0].options());
  launch_embed_fwd(tabs, (int)weights.size(), (int)T, (int)D, (int)S, bf(out), cur_stream());
  return out;
}

// grads: fp32 [V, D] slots accumulated into (zero them first for a fresh gradient)
void embed_bwd(Tensor g, std::vector<Tensor> grads, std::vector<c10::optional<Tensor>> ids, int64_t S) {
  check_bf16(g, "g");
  TORCH_CHECK(g.dim() == 2, "g must be [T, D]");
  TORCH_CHECK(!grads.empty() && grads.size() <= 3 && grads.size() == ids.size(), "1-3 tables, one ids each");
  const long T = g.size(0), D = g.size(1);
  k8s_amd::EmbTable tabs[3];
  for (size_t i = 0; i < grads.size(); ++i) {
    const Tensor& gr = grads[i];
    check_cuda(gr, "grad"); check_dtype(gr, at::kFloat, "grad");
    TORCH_CHECK(gr.dim() == 2 && gr.size(1) == D, "grad slots must be [V, D]");
    tabs[i] = k8s_amd::EmbTable{nullptr, f32(gr), embed_ids(ids[i], T, S, gr.size(0)), (int)gr.size(0)};
  }
  launch_embed_bwd(tabs, (int)grads.size(), (int)T, (int)D, (int)S, cbf(g), cur_stream());
}

// ------------------------------------------------------------------ space-to-depth stem
// y[n][i][j] = x[n][s i][s j]: the input of a 1x1 / stride-s / pad-0 convolution as a contiguous tensor
Tensor subsample_nhwc(Tensor x, int64_t s) {
  check_bf16(x, "x");
  TORCH_CHECK(x.dim() == 4 && x.size(3) % 8 == 0 && s >= 1, "x: contiguous NHWC, C % 8 == 0");
  const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  auto y = torch::empty({N, (H + s - 1) / s, (W + s - 1) / s, C}, x.options());
  launch_subsample_nhwc(cbf(x), bf(y), N, H, W, C, (int)s, cur_stream());
  return y;
}
Tensor stem_s2d_input(Tensor x, int64_t pad) {
  check_bf16(x, "x");
  TORCH_CHECK(x.dim() == 4 && x.size(3) <= 8 && pad >= 0, "x must be NHWC with <= 8 channels");
  const int N = x.size(0), H = x.size(1), W = x.size(2);
  auto out = torch::empty({N, (H + 2 * pad) / 2, (W + 2 * pad) / 2, 16}, x.options());
  launch_stem_s2d_input(cbf(x), N, H, W, (int)x.size(3), (int)pad, bf(out), cur_stream());
  return out;
}
Tensor stem_w_s2d(Tensor w7) {
  check_bf16(w7, "w7");
  TORCH_CHECK(w7.dim() == 4 && w7.size(1) == w7.size(2), "w7 must be [K, R, R, C]");
  const int K = w7.size(0), R = w7.size(1), Rs = (R + 1) / 2;
  auto w4 = torch::empty({K, Rs, Rs, 16}, w7.options());
  launch_stem_w_s2d(cbf(w7), K, R, (int)w7.size(3), bf(w4), cur_stream());
  return w4;
}
// the s2d stem convolution on its LDS-tiled kernel (stem.hip): y [N, Hs-3, Ws-3, 64] + BN statistics into `stats`
Tensor stem_conv_fwd(Tensor xs, Tensor w4, Tensor stats) {
  check_bf16(xs, "xs"); check_bf16(w4, "w4");
  TORCH_CHECK(xs.dim() == 4 && xs.size(3) == 16, "xs must be a contiguous [N, Hs, Ws, 16] image");
  TORCH_CHECK(w4.dim() == 4 && k8s_amd::stem_conv_fwd_ok((int)w4.size(0), (int)w4.size(1), (int)w4.size(3),
              (int)xs.size(2) - 3) && w4.size(2) == 4, "stem conv: w4 [64, 4, 4, 16], Wo % 16 == 0");
  check_stat_sums(stats, 64, "stats", true);
  const int N = xs.size(0), Hs = xs.size(1), Ws = xs.size(2);
  auto y = torch::empty({N, Hs - 3, Ws - 3, 64}, xs.options());
  launch_stem_conv_fwd(cbf(xs), cbf(w4), bf(y), f32(stats), N, Hs, Ws, cur_stream());
  return y;
}

// the s2d stem weight gradient (stem.hip): dw4 fp32 [64, 4, 4, 16] from the image xs and the output gradient dy
void stem_wgrad(Tensor xs, Tensor dy, Tensor dw4) {
  check_bf16(xs, "xs"); check_bf16(dy, "dy");
  TORCH_CHECK(xs.dim() == 4 && xs.size(3) == 16, "xs [N, Hs, Ws, 16]");
  const int N = xs.size(0), Hs = xs.size(1), Ws = xs.size(2);
  TORCH_CHECK(dy.dim() == 4 && dy.size(0) == N && dy.size(1) == Hs - 3 && dy.size(2) == Ws - 3 && dy.size(3) == 64 &&
              k8s_amd::stem_conv_fwd_ok(64, 4, 16, Ws - 3), "dy [N, Hs-3, Ws-3, 64], Wo % 16 == 0");
  check_channel_f32(dw4, 64 * 256, "dw4");
  auto ws = torch::empty({(long)k8s_amd::stem_wgrad_blocks(N, Hs) * 64 * 256}, dw4.options());
  launch_stem_wgrad(cbf(xs), cbf(dy), f32(ws), f32(dw4), N, Hs, Ws, cur_stream());
}
void stem_dw_s2d(Tensor dw4, Tensor dw7) {
  check_cuda(dw4, "dw4"); check_cuda(dw7, "dw7");
  check_dtype(dw4, at::kFloat, "dw4"); check_dtype(dw7, at::kFloat, "dw7");
  TORCH_CHECK(dw7.dim() == 4 && dw7.size(1) == dw7.size(2), "dw7 must be [K, R, R, C]");
  const int K = dw7.size(0), R = dw7.size(1), Rs = (R + 1) / 2;
  TORCH_CHECK(dw4.numel() == (long)K * Rs * Rs * 16, "dw4 must be [K, Rs, Rs, 16]");
  launch_stem_dw_s2d(f32(dw4), K, R, (int)dw7.size(3), f32(dw7), cur_stream());
}

}  // namespace

void bind_elementwise(pybind11::module_& m) {
  m.def("mask_apply", &mask_apply, "out = bit ? src : 0 (packed 1-bit mask per element)");
  m.def("swiglu_fwd", &swiglu_fwd, "gu"_a, "blk"_a = 0);
  m.def("swiglu_bwd", &swiglu_bwd, "gu"_a, "dy"_a, "blk"_a = 0);
  m.def("rope_", &rope_);
  m.def("gelu_bwd", &gelu_bwd);
  m.def("relu_bwd", &relu_bwd);
  m.def("colsum", &colsum, "x"_a, "out"_a = py::none());
  m.def("act_bwd_colsum", &act_bwd_colsum, "dy"_a, "pre"_a, "act"_a, "out"_a = py::none());
  m.def("maxpool_fwd", &maxpool_fwd);
  m.def("maxpool_bwd", &maxpool_bwd);
  m.def("avgpool_fwd", &avgpool_fwd);
  m.def("avgpool_bwd", &avgpool_bwd);
  m.def("embed_fwd", &embed_fwd);
  m.def("embed_bwd", &embed_bwd);
  m.def("subsample_nhwc", &subsample_nhwc, "x"_a, "s"_a);
  m.def("stem_s2d_input", &stem_s2d_input);
  m.def("stem_w_s2d", &stem_w_s2d);
  m.def("stem_conv_fwd", &stem_conv_fwd);
  m.def("stem_wgrad", &stem_wgrad);
  m.def("stem_dw_s2d", &stem_dw_s2d);
}

}  // namespace k8s_amd::binding
