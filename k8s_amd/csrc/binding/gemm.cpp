// GEMM (MFMA): the general product, the 4-wave 256 x 256 kernel's epilogue forms (SwiGLU, rotary embedding,
// activation backward) and the 1x1 data gradients that also take a BatchNorm's backward sums.
#include "binding/common.h"

#include <algorithm>
#include <map>
#include <mutex>
#include <utility>

namespace k8s_amd::binding {

int gemm256_mode() {
  const char* e = std::getenv("K8S_AMD_GEMM256");
  return e ? atoi(e) : 1;
}
bool use_gemm256(long M, long N, long K, bool a_kmajor, bool b_kmajor) {
  const int m = gemm256_mode();
  if (m == 2)
    return K % 64 == 0 && N % 4 == 0 && (a_kmajor || M % 8 == 0) && (b_kmajor || N % 8 == 0);
  return m != 0 && gemm256_eligible((int)M, (int)N, (int)K, a_kmajor, b_kmajor);
}

// Grown on demand. The kernel leaves every word it used at zero again, so no per-call clear is needed; launches on one
// stream are ordered, so they never share the words concurrently, and two streams (a side stream, user streams) get
// their own.
int* sk_sync_words(long n, const c10::Device& dev) {
  static std::mutex mu;
  static std::map<std::pair<int, int64_t>, Tensor> bufs;
  const int64_t sid = at::hip::getCurrentHIPStream(dev.index()).id();
  std::lock_guard<std::mutex> g(mu);
  Tensor& t = bufs[{dev.index(), sid}];
  if (!t.defined() || t.numel() < n)
    t = torch::zeros({std::max<long>(n, 1 << 16)}, torch::TensorOptions().dtype(at::kInt).device(dev));
  return t.data_ptr<int>();
}
SkScratch::SkScratch(const Gemm256Plan& plan, const Tensor& like) {
  if (plan.sk <= 1) return;
  slabs = torch::empty({gemm256_sk_slab_floats(plan)}, like.options().dtype(at::kFloat));
  sync = sk_sync_words(gemm256_sk_sync_ints(plan), like.device());
}

namespace {

// 2-D bf16 GPU rows with unit column stride, 16-byte aligned, leading dimension % 8 == 0
void check_bf16_operand(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 2 && t.stride(1) == 1, name, " must be a 2-D row-major GPU tensor");
  check_dtype(t, at::kBFloat16, name);
  check_aligned(t, name);
  TORCH_CHECK(t.stride(0) % 8 == 0, name, " leading dimension must be a multiple of 8 elements");
}

// 1x1 data gradient dx[M, N] = gy[M, K] . w[K, N] + (add_mask ? add_src : 0) that also accumulates the
// BatchNorm-backward statistics of dx for the BatchNorm(s) that produced the convolution's input (gemm_short.hip
// EPI 3 / 4): sums[r][0][c] += sum g, sums[r][1][c] += sum g (x - mean), g = bit ? dx : 0 with the BatchNorm's packed
// ReLU bits `mask`; with x2 (a ResNet downsample block's second BatchNorm) sums2[r][1][c] += sum g (x2 - mean2).
// sums / sums2: zeroed fp32 [conv_stat_replicas, 2, N].
Tensor dgrad_short_bnstats(Tensor gy, Tensor w, OptTensor add_src, OptTensor add_mask, Tensor x, Tensor mask,
                           Tensor mean, Tensor sums, OptTensor x2, OptTensor mean2, OptTensor sums2) {
  // no addend (add_src None): the plain data gradient + the sums (EPI 5), one BatchNorm only
  const bool has_add = add_src.has_value();
  TORCH_CHECK(has_add == add_mask.has_value() && (has_add || !x2), "add_src / add_mask together; x2 needs them");
  check_bf16_dense(gy, 2, "gy"); check_bf16_dense(w, 2, "w"); check_bf16_dense(x, 2, "x");
  const long M = gy.size(0), K = gy.size(1), N = w.size(1);
  TORCH_CHECK(w.size(0) == K && x.size(0) == M && x.size(1) == N, "shapes: gy [M, K], w [K, N], add_src / x [M, N]");
  TORCH_CHECK(M < (1L << 31) && k8s_amd::gemm_short_bnstats_ok((int)M, (int)N, (int)K, x2.has_value()),
              "dgrad_short_bnstats: shape outside the kernel's contract (gemm_short_bnstats_ok)");
  const uint8_t* am = nullptr;
  if (has_add) {
    check_bf16_dense(*add_src, 2, "add_src");
    TORCH_CHECK(add_src->sizes() == x.sizes(), "add_src: [M, N]");
    am = check_bit_mask(*add_mask, M * N, "add_mask");
  }
  const k8s_amd::GemmShortBnStats b = gemm_short_bn_stats(x, mask, mean, sums, x2, mean2, sums2);
  Tensor out = torch::empty({M, N}, gy.options());
  launch_gemm_short(cbf(gy), cbf(w), N, true, bf(out), has_add ? cbf(*add_src) : nullptr, am, nullptr, nullptr, (int)M,
                    (int)N, (int)K, has_add ? 2 : 0, cur_stream(), &b);
  return out;
}

// 1x1 data gradient dx[M, N] = gy[M, K] . w[K, N] on the tile kernel with the BatchNorm-backward sums of dx for the
// relu(BN(x)) that produced the convolution's input (gemm.hip TileEpi::LeanBnBwd); for shapes the 4-wave kernel does not
// take (gemm_dgrad_bnstats_ok). sums: zeroed fp32 [conv_stat_replicas, 2, N].
Tensor gemm_dgrad_bnstats(Tensor gy, Tensor w, Tensor x, Tensor gamma, Tensor beta, Tensor mean, Tensor invstd,
                          Tensor sums) {
  check_bf16_dense(gy, 2, "gy"); check_bf16_dense(w, 2, "w"); check_bf16_dense(x, 2, "x");
  const long M = gy.size(0), K = gy.size(1), N = w.size(1);
  TORCH_CHECK(w.size(0) == K && x.size(0) == M && x.size(1) == N, "shapes: gy [M, K], w [K, N], x [M, N]");
  TORCH_CHECK(N % 8 == 0 && M < (1L << 31), "N % 8 == 0");
  const k8s_amd::BnBwdSums bb = bn_bwd_sums(x, mean, sums, {}, gamma, beta, invstd, {}, {}, {});
  const bool w4 = use_gemm256(M, N, K, true, false);  // the product's regular path is the 256 x 256 kernel: its epilogue
  TORCH_CHECK(!w4 || k8s_amd::gemm_w4_dgrad_bnstats_ok((int)M, (int)N, (int)K), "gemm_dgrad_bnstats: 4-wave contract");
  Tensor out = torch::empty({M, N}, gy.options());
  if (w4) {
    Tensor tab = torch::cat({gamma, beta, mean, invstd});
    const SkScratch sk(k8s_amd::gemm256_plan((int)M, (int)N, (int)K), gy);
    launch_gemm_w4_dgrad_bnstats(cbf(gy), cbf(w), bf(out), (int)M, (int)N, (int)K, cbf(x), f32(tab), f32(sums),
                                 sk.slab_ptr(), sk.sync_ptr(), cur_stream());
    return out;
  }
  launch_gemm_dgrad_bnstats(cbf(gy), cbf(w), bf(out), (int)M, (int)N, (int)K, bb, cur_stream());
  return out;
}

// out[M, N] += gy[M, K] . w[K, N] on the tile kernel, also accumulating the BatchNorm-backward sums of the final out
// for a BatchNorm whose ReLU bits are stored (mask kind: g = bit ? out : 0, sum g, sum g (x - mean)) -- the second
// of two data gradients into that BatchNorm's output (the stem pool's, nn.BnStatLink.last_full). Returns out.
// With add_src / add_mask (a ResNet identity block's residual gradient as (dy, packed ReLU bits)): out = product +
// (bit ? add_src : 0), out's old values unread.
// x2 / mean2 / sums2: the two-BatchNorm form (a ResNet downsample block's output), sums2[.][1] += sum g (x2 - mean2).
Tensor gemm_dgrad_bnstats_mask(Tensor gy, Tensor w, Tensor out, Tensor x, Tensor mask, Tensor mean, Tensor sums,
                               OptTensor add_src, OptTensor add_mask, OptTensor x2, OptTensor mean2, OptTensor sums2) {
  for (const Tensor* t : {&gy, &w, &out, &x}) check_bf16_dense(*t, 2, "gy / w / out / x");
  const long M = gy.size(0), K = gy.size(1), N = w.size(1);
  TORCH_CHECK(w.size(0) == K && x.size(0) == M && x.size(1) == N && out.sizes() == x.sizes(),
              "shapes: gy [M, K], w [K, N], out / x [M, N]");
  TORCH_CHECK(N % 8 == 0 && M < (1L << 31), "N % 8 == 0");
  TORCH_CHECK(x2.has_value() == mean2.has_value() && x2.has_value() == sums2.has_value(), "x2 / mean2 / sums2 together");
  const k8s_amd::BnBwdSums bb = bn_bwd_sums(x, mean, sums, mask, {}, {}, {}, x2, mean2, sums2);
  TORCH_CHECK(add_src.has_value() == add_mask.has_value(), "add_src and add_mask together");
  const uint8_t* am = nullptr;
  if (add_src) {
    check_bf16_dense(*add_src, -1, "add_src");
    TORCH_CHECK(add_src->numel() == M * N, "add_src: [M, N]");
    am = check_bit_mask(*add_mask, M * N, "add_mask");
  }
  launch_gemm_dgrad_bnstats(cbf(gy), cbf(w), bf(out), (int)M, (int)N, (int)K, bb, cur_stream(), true,
                            add_src ? cbf(*add_src) : nullptr, am);
  return out;
}

// The tile kernel's form for a launch described by plain values (gemm.hip choose_tile_form): a pure host function,
// like flash_plan. A launch the chooser refuses raises its message.
std::string gemm_tile_form(const std::string& pair, int64_t wm, int64_t N, int64_t splits, int64_t xuse, int64_t ldc,
                           bool out_f32, int64_t mode, bool bias, bool pre, int64_t act, bool stats, bool rst,
                           bool addsrc, bool addmask, bool bb_sums, bool bb_mask, bool c_aligned, bool pre_aligned) {
  k8s_amd::TileFormQuery q;
  q.pair = pair.c_str(); q.wm = (int)wm; q.N = (int)N; q.splits = (int)splits; q.xuse = (int)xuse;
  q.ldc = ldc < 0 ? N : ldc; q.out_f32 = out_f32; q.mode = (int)mode; q.act = (int)act;
  q.bias = bias; q.pre = pre; q.stats = stats; q.rst = rst; q.addsrc = addsrc; q.addmask = addmask;
  q.bb_sums = bb_sums; q.bb_mask = bb_mask; q.c_aligned = c_aligned; q.pre_aligned = pre_aligned;
  return k8s_amd::gemm_tile_form(q);
}

bool gemm_dgrad_bnstats_ok(int64_t M, int64_t N, int64_t K) {
  const char* e = std::getenv("K8S_AMD_BN_BSTATS");
  if (e && e[0] == '0') return false;
  if (M >= (1L << 31) || N % 8 != 0) return false;
  if (use_gemm256(M, N, K, true, false)) {
    const char* g = std::getenv("K8S_AMD_BN_BSTATS_W4");
    return !(g && g[0] == '0') && k8s_amd::gemm_w4_dgrad_bnstats_ok((int)M, (int)N, (int)K);
  }
  return !k8s_amd::gemm_short_ok((int)M, (int)N, (int)K, K, N);
}

// a: [M,K] if a_kmajor else [K,M];  b: [N,K] if b_kmajor else [K,N];  returns / writes C[M,N]
Tensor gemm(Tensor a, bool a_kmajor, Tensor b, bool b_kmajor, OptTensor out, bool out_f32, OptTensor bias, int64_t act,
            OptTensor pre, bool accumulate, double alpha, int64_t splits, OptTensor add_src, OptTensor add_mask,
            OptTensor xform_b, int64_t xform_c) {
  check_bf16_operand(a, "A"); check_bf16_operand(b, "B");
  const long M = a_kmajor ? a.size(0) : a.size(1), K = a_kmajor ? a.size(1) : a.size(0);
  const long N = b_kmajor ? b.size(0) : b.size(1), Kb = b_kmajor ? b.size(1) : b.size(0);
  TORCH_CHECK(K == Kb, "inner dimensions differ: ", K, " vs ", Kb);
  // a K-major operand's K % 64 tail reads zeros (KMajor::ktot; e.g. the 1000-class head's data gradient)
  TORCH_CHECK((a_kmajor ? K : M) % 8 == 0 && (b_kmajor ? K : N) % 8 == 0 && N % 4 == 0,
              "each operand's contiguous dimension (K if K-major, else M / N) must be a multiple of 8, N of 4");
  if (out) {
    TORCH_CHECK(out->is_cuda() && out->is_contiguous() && out->numel() == M * N, "out must be a contiguous [M,N] tensor");
    TORCH_CHECK(out->scalar_type() == (out_f32 ? at::kFloat : at::kBFloat16), "out dtype mismatch");
  }
  if (bias) check_channel_f32(*bias, N, "bias");
  if (pre) {
    check_bf16_dense(*pre, -1, "pre");
    TORCH_CHECK(pre->numel() == M * N, "pre: the output's size");
  }
  const int mode = accumulate ? 1 : 0;
  k8s_amd::AddEpi add{nullptr, nullptr};
  if (add_src) {
    TORCH_CHECK(accumulate && !out_f32, "add_src: a bf16 accumulate-mode output");
    check_bf16_dense(*add_src, -1, "add_src");
    TORCH_CHECK(add_src->numel() == M * N, "add_src must be a contiguous bf16 tensor of the output's size");
    add.src = cbf(*add_src);
    if (add_mask) add.mask = check_bit_mask(*add_mask, M * N, "add_mask");
  } else {
    TORCH_CHECK(!add_mask, "add_mask needs add_src");
  }
  const float* xfb = xform_ptr(xform_b, xform_c);
  if (xfb) TORCH_CHECK(!a_kmajor && !b_kmajor && out_f32 && !bias && act == 0 && !pre && !add_src &&
                           N % xform_c == 0, "normalize-on-load GEMM: the plain weight-gradient form only");
  Tensor c = out ? *out : torch::empty({M, N}, a.options().dtype(out_f32 ? at::kFloat : at::kBFloat16));
  if (!xfb && !add_src && use_gemm256(M, N, K, a_kmajor, b_kmajor)) {
    const SkScratch sk(k8s_amd::gemm256_plan((int)M, (int)N, (int)K), a);
    launch_gemm256(cbf(a), a.stride(0), a_kmajor, cbf(b), b.stride(0), b_kmajor, c.data_ptr(), N, out_f32, (int)M,
                   (int)N, (int)K, optf(bias), (int)act, pre ? bf(*pre) : nullptr, accumulate, (float)alpha,
                   cur_stream(), 1, nullptr, sk.slab_ptr(), sk.sync_ptr());
    return c;
  }
  // tall-K fp32 products whose output is too small for the 256 x 256 kernel alone (the ResNet 1x1 weight gradients):
  // split-K on the 256 kernel
  if (!xfb && !add_src && splits != 1 && out_f32 && !bias && act == 0 && !pre && gemm256_mode() != 0 &&
      K % 64 == 0 && (a_kmajor || M % 8 == 0) && (b_kmajor || N % 8 == 0) && N % 4 == 0) {
    const int s256 = k8s_amd::gemm256_choose_splits((int)M, (int)N, (int)K);
    const long t256 = ((M + 255) / 256) * ((N + 255) / 256);
    if (s256 > 1 && t256 * s256 >= 128) {
      auto ws = torch::empty({(long)s256 * M * N}, c.options());
      launch_gemm256(cbf(a), a.stride(0), a_kmajor, cbf(b), b.stride(0), b_kmajor, c.data_ptr(), N, true, (int)M,
                     (int)N, (int)K, nullptr, 0, nullptr, accumulate, (float)alpha, cur_stream(), s256, f32(ws));
      return c;
    }
  }
  int sp = (int)splits;
  if (sp != 1 && out_f32 && !bias && act == 0 && !pre && N % 4 == 0) {
    if (sp <= 0) sp = k8s_amd::gemm_choose_splits((int)M, (int)N, (int)K);
  } else {
    sp = 1;
  }
  Tensor ws;
  if (sp > 1) ws = torch::empty({k8s_amd::gemm_splitk_workspace((int)M, (int)N, sp)}, a.options().dtype(at::kFloat));
  launch_gemm(cbf(a), a.stride(0), a_kmajor, cbf(b), b.stride(0), b_kmajor, c.data_ptr(), N, out_f32, (int)M, (int)N,
              (int)K, optf(bias), (int)act, pre ? bf(*pre) : nullptr, mode, (float)alpha, sp,
              sp > 1 ? f32(ws) : nullptr, cur_stream(), add_src ? &add : nullptr, xfb, (int)xform_c);
  return c;
}

// Llama's down-projection data gradient fused with the SwiGLU backward: dgu [M, 2F] = swiglu_bwd(gu, g . w),
// g [M, K] bf16, w [K, F] bf16 (the down weight [out, in], read MN-major), gu [M, 2F] bf16 (gate | up).
bool gemm_swiglu_bwd_ok(int64_t M, int64_t F, int64_t K) { return gemm_w4_swiglu_ok((int)M, (int)F, (int)K, K, F); }
Tensor gemm_swiglu_bwd(Tensor g, Tensor w, Tensor gu, int64_t blk) {
  check_bf16_operand(g, "g"); check_bf16_operand(w, "w"); check_bf16_operand(gu, "gu");
  const long M = g.size(0), K = g.size(1), F = w.size(1);
  TORCH_CHECK(w.size(0) == K, "g [M, K] . w [K, F]");
  TORCH_CHECK(gu.is_contiguous() && gu.size(0) == M && gu.size(1) == 2 * F, "gu must be a contiguous [M, 2F]");
  TORCH_CHECK(k8s_amd::gemm_w4_swiglu_ok((int)M, (int)F, (int)K, g.stride(0), w.stride(0)),
              "gemm_swiglu_bwd: shape outside the 4-wave kernel's contract");
  TORCH_CHECK(blk == 0 || blk == 64, "gemm_swiglu_bwd: blk is 0 (gate | up halves) or 64 (blocked layout)");
  Tensor dgu = torch::empty({M, 2 * F}, g.options());
  const SkScratch sk(k8s_amd::gemm256_plan((int)M, (int)F, (int)K), g);
  launch_gemm_w4_swiglu_bwd(cbf(g), g.stride(0), cbf(w), w.stride(0), bf(dgu), cbf(gu), (int)M, (int)F, (int)K,
                            (int)blk, sk.slab_ptr(), sk.sync_ptr(), cur_stream());
  return dgu;
}

// Llama's QKV projection with the rotary embedding of its q / k heads (the first rot_cols columns, head dim 128) in
// the epilogue: y [M, N] = x [M, K] . w [N, K]^T, pos [M] int32, table [maxpos, 64, 2] fp32 (gemm256.hip copy_out_rope)
bool gemm_rope_ok(int64_t M, int64_t N, int64_t K, int64_t rot_cols) {
  return k8s_amd::gemm_w4_rope_ok((int)M, (int)N, (int)K, K, K, (int)rot_cols);
}
Tensor gemm_rope(Tensor x, Tensor w, Tensor pos, Tensor table, int64_t rot_cols) {
  check_bf16_operand(x, "x"); check_bf16_operand(w, "w");
  const long M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "x [M, K] . w [N, K]^T, row-major");
  TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == at::kInt && pos.is_contiguous() && pos.numel() == M, "pos: [M] int32");
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == at::kFloat && table.is_contiguous() && table.dim() == 3 &&
                  table.size(1) == 64 && table.size(2) == 2, "table: [maxpos, 64, 2] fp32 (head dim 128)");
  TORCH_CHECK(k8s_amd::gemm_w4_rope_ok((int)M, (int)N, (int)K, x.stride(0), w.stride(0), (int)rot_cols),
              "gemm_rope: shape outside the 4-wave kernel's contract");
  Tensor y = torch::empty({M, N}, x.options());
  const SkScratch sk(k8s_amd::gemm256_plan((int)M, (int)N, (int)K), x);
  launch_gemm_w4_rope(cbf(x), x.stride(0), cbf(w), w.stride(0), bf(y), (int)M, (int)N, (int)K, pos.data_ptr<int>(),
                      f32(table), (int)rot_cols, sk.slab_ptr(), sk.sync_ptr(), cur_stream());
  return y;
}

// Llama's gate|up projection with the SwiGLU in the epilogue: returns (gu [M, 2F], h [M, F] = silu(gate) up) from
// x [M, K] bf16 and w [2F, K] bf16 whose rows are in the 64-blocked gate|up order (gemm256.hip copy_out_swiglu).
bool gemm_swiglu_fwd_ok(int64_t M, int64_t F, int64_t K) { return gemm_w4_swiglu_fwd_ok((int)M, (int)F, (int)K, K, K); }
std::vector<Tensor> gemm_swiglu_fwd(Tensor x, Tensor w) {
  check_bf16_operand(x, "x"); check_bf16_operand(w, "w");
  const long M = x.size(0), K = x.size(1), F2 = w.size(0);
  TORCH_CHECK(w.size(1) == K && F2 % 2 == 0, "x [M, K] . w [2F, K]^T");
  const long F = F2 / 2;
  TORCH_CHECK(k8s_amd::gemm_w4_swiglu_fwd_ok((int)M, (int)F, (int)K, x.stride(0), w.stride(0)),
              "gemm_swiglu_fwd: shape outside the 4-wave kernel's contract");
  Tensor gu = torch::empty({M, F2}, x.options());
  Tensor h = torch::empty({M, F}, x.options());
  const SkScratch sk(k8s_amd::gemm256_plan((int)M, (int)F2, (int)K), x);
  launch_gemm_w4_swiglu_fwd(cbf(x), x.stride(0), cbf(w), w.stride(0), bf(gu), bf(h), (int)M, (int)F, (int)K,
                            sk.slab_ptr(), sk.sync_ptr(), cur_stream());
  return {gu, h};
}

// dx = (g . W) * act'(pre) and db (+)= column sums of dx: the data gradient of a linear whose input is the output of
// an activation (1 ReLU: pre = the ReLU output, 2 GELU: the pre-activation), fused with that activation's backward and
// the producing linear's bias gradient in the 4-wave GEMM's epilogue (gemm256.hip copy_out_x, ACT < 0).
// g [M, N_out] bf16, w [N_out, K_in] bf16 (read MN-major), pre [M, K_in] bf16, db fp32 [K_in].
bool gemm_dact_ok(int64_t M, int64_t N, int64_t K) { return k8s_amd::gemm_w4_dact_ok((int)M, (int)N, (int)K, K, N, N); }
Tensor gemm_dact(Tensor g, Tensor w, Tensor pre, int64_t act, Tensor db, bool db_accumulate) {
  check_bf16_operand(g, "g"); check_bf16_operand(w, "w"); check_bf16_operand(pre, "pre");
  const long M = g.size(0), K = g.size(1), N = w.size(1);
  TORCH_CHECK(w.size(0) == K, "g [M, K] . w [K, N]");
  TORCH_CHECK(pre.is_contiguous() && pre.size(0) == M && pre.size(1) == N, "pre must be a contiguous [M, N]");
  check_channel_f32(db, N, "db");
  TORCH_CHECK(act == 1 || act == 2, "act: 1 ReLU, 2 GELU(tanh)");
  TORCH_CHECK(k8s_amd::gemm_w4_dact_ok((int)M, (int)N, (int)K, g.stride(0), w.stride(0), N),
              "gemm_dact: shape outside the 4-wave kernel's contract");
  Tensor c = torch::empty({M, N}, g.options());
  Tensor part = torch::empty({k8s_amd::gemm_w4_dact_part_floats((int)M, (int)N)}, db.options());
  const SkScratch sk(k8s_amd::gemm256_plan((int)M, (int)N, (int)K), g);
  launch_gemm_w4_dact(cbf(g), g.stride(0), cbf(w), w.stride(0), bf(c), N, (int)M, (int)N, (int)K, cbf(pre), (int)act,
                      f32(part), f32(db), db_accumulate, sk.slab_ptr(), sk.sync_ptr(), cur_stream());
  return c;
}

}  // namespace

void bind_gemm(pybind11::module_& m) {
  m.def("gemm", &gemm, "a"_a, "a_kmajor"_a, "b"_a, "b_kmajor"_a, "out"_a, "out_f32"_a, "bias"_a, "act"_a, "pre"_a,
        "accumulate"_a, "alpha"_a, "splits"_a, "add_src"_a = py::none(), "add_mask"_a = py::none(),
        "xform_b"_a = py::none(), "xform_c"_a = 0);
  m.def("gemm_tile_form", &gemm_tile_form, "pair"_a, "wm"_a = 2, "N"_a = 128, "splits"_a = 1, "xuse"_a = 0, "ldc"_a = -1,
        "out_f32"_a = false, "mode"_a = 0, "bias"_a = false, "pre"_a = false, "act"_a = 0, "stats"_a = false,
        "rst"_a = false, "addsrc"_a = false, "addmask"_a = false, "bb_sums"_a = false, "bb_mask"_a = false,
        "c_aligned"_a = true, "pre_aligned"_a = true,
        "which form of the tile kernel (gemm.hip TileEpi, +A / +B on-load) a launch takes; ldc < 0: N");
  m.def("gemm_short_ok", [](int64_t M, int64_t N, int64_t K) { return k8s_amd::gemm_short_ok((int)M, (int)N, (int)K, K, N); },
        "whether C[M,N] = A[M,K] . B^T (contiguous) takes the short-K streaming kernel (gemm_short.hip)");
  m.def("dgrad_short_bnstats", &dgrad_short_bnstats, "gy"_a, "w"_a, "add_src"_a, "add_mask"_a, "x"_a, "mask"_a,
        "mean"_a, "sums"_a, "x2"_a = py::none(), "mean2"_a = py::none(), "sums2"_a = py::none(),
        "1x1 masked-addend data gradient with the BatchNorm-backward statistics of its result (gemm_short EPI 3/4)");
  m.def("gemm_short_bnstats_ok", [](int64_t M, int64_t N, int64_t K, bool dual) {
    return M < (1L << 31) && k8s_amd::gemm_short_bnstats_ok((int)M, (int)N, (int)K, dual);
  });
  m.def("gemm_dgrad_bnstats", &gemm_dgrad_bnstats,
        "1x1 data gradient with the BatchNorm-backward sums of a relu(BN(x)) input (gemm.hip TileEpi::LeanBnBwd)");
  m.def("gemm_dgrad_bnstats_ok", &gemm_dgrad_bnstats_ok,
        "whether a 1x1 data gradient takes gemm_dgrad_bnstats (on its regular kernel: the 4-wave or the tile kernel)");
  m.def("gemm_dgrad_bnstats_mask", &gemm_dgrad_bnstats_mask, "gy"_a, "w"_a, "out"_a, "x"_a, "mask"_a, "mean"_a,
        "sums"_a, "add_src"_a = py::none(), "add_mask"_a = py::none(), "x2"_a = py::none(), "mean2"_a = py::none(),
        "sums2"_a = py::none());
  m.def("gemm_dact", &gemm_dact, "linear data gradient fused with the input activation's backward and bias gradient",
        "g"_a, "w"_a, "pre"_a, "act"_a, "db"_a, "db_accumulate"_a);
  m.def("gemm_dact_ok", &gemm_dact_ok, "M"_a, "N"_a, "K"_a);
  m.def("gemm_swiglu_bwd", &gemm_swiglu_bwd, "down-projection data gradient fused with the SwiGLU backward (dgu)",
        "g"_a, "w"_a, "gu"_a, "blk"_a = 0);
  m.def("gemm_swiglu_bwd_ok", &gemm_swiglu_bwd_ok, "M"_a, "F"_a, "K"_a);
  m.def("gemm_swiglu_fwd", &gemm_swiglu_fwd, "gate|up projection with the SwiGLU in the epilogue: (gu, h)");
  m.def("gemm_swiglu_fwd_ok", &gemm_swiglu_fwd_ok, "M"_a, "F"_a, "K"_a);
  m.def("gemm_rope", &gemm_rope, "QKV projection with the q / k rotary embedding in the epilogue");
  m.def("gemm_rope_ok", &gemm_rope_ok, "M"_a, "N"_a, "K"_a, "rot_cols"_a);
}

}  // namespace k8s_amd::binding
