// Generation entry points of k8s_amd._C (kernels/decode.hip): the skinny-M weight-streaming GEMM, the KV-cache append
// and the split-key decode attention. Device tables (start, lens) come with the host mirror the caller keeps: the
// mirror is validated here, before anything is allocated or launched, and the kernels clamp the device copy once more.
#include <algorithm>

#include "binding/common.h"

namespace k8s_amd::binding {
namespace {

long g_decode_launches = 0;  // launcher calls so far: the tests check that a rejected call never got this far

// x bf16 [M, K], 1 <= M <= 16; w bf16 [N, K] (K-major, as the flat store keeps it); K % 64 == 0, N % 16 == 0
Tensor linear_skinny(Tensor x, Tensor w) {
  check_bf16_dense(x, 2, "x");
  check_bf16_dense(w, 2, "w");
  TORCH_CHECK(x.device() == w.device(), "x and w must be on one device");
  const long M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "w must be [N, K = ", K, "], got [", N, ", ", w.size(1), "]");
  TORCH_CHECK(k8s_amd::linear_skinny_ok(M, N, K), "linear_skinny takes 1 <= M <= 16, K % 64 == 0 and N % 16 == 0, got "
              "M = ", M, ", N = ", N, ", K = ", K);
  const SkinnyPlan p = k8s_amd::skinny_plan(N, K);
  auto y = torch::empty({M, N}, x.options());
  Tensor part;
  if (p.nsplit > 1) part = torch::empty({p.nsplit, M, N}, x.options().dtype(at::kFloat));
  ++g_decode_launches;
  launch_linear_skinny(cbf(x), cbf(w), bf(y), p.nsplit > 1 ? f32(part) : nullptr, (int)M, (int)N, (int)K,
                       cur_stream());
  return y;
}

// the caches of one layer: bf16 [B, Hkv, Smax, D] each. Returns (B, Hkv, Smax, D).
std::array<long, 4> check_caches(const Tensor& ck, const Tensor& cv) {
  check_bf16_dense(ck, 4, "cache_k");
  check_bf16_dense(cv, 4, "cache_v");
  TORCH_CHECK(ck.sizes() == cv.sizes() && ck.device() == cv.device(), "cache_k and cache_v must have one shape and "
              "device");
  TORCH_CHECK(ck.size(0) >= 1 && ck.size(1) >= 1 && ck.size(2) >= 1 && ck.size(3) >= 8 && ck.size(3) % 8 == 0,
              "caches must be [B, Hkv, Smax, D] with D a multiple of 8");
  TORCH_CHECK(ck.size(2) < (1L << 24) && ck.numel() < (1L << 40), "cache too large");
  return {ck.size(0), ck.size(1), ck.size(2), ck.size(3)};
}

// a device int32 [B] table and its host mirror
const int32_t* check_table(const Tensor& dev, const Tensor& host, long B, const Tensor& like, const char* name) {
  check_cuda(dev, name);
  check_dtype(dev, at::kInt, name);
  TORCH_CHECK(dev.dim() == 1 && dev.size(0) == B && dev.device() == like.device(), name, " must be int32 [B = ", B,
              "] on the caches' device");
  TORCH_CHECK(host.device().is_cpu(), name, ": the host mirror must be a CPU tensor");
  check_dtype(host, at::kInt, name);
  TORCH_CHECK(host.dim() == 1 && host.size(0) == B && host.is_contiguous(), name, ": the host mirror must be a "
              "contiguous int32 [B = ", B, "]");
  return host.data_ptr<int32_t>();
}

// qkv bf16 [B * S, (Hq + 2 Hkv) * D], packed and already rotated; token s of row b -> cache position start[b] + s
void kv_append(Tensor qkv, Tensor cache_k, Tensor cache_v, Tensor start, Tensor start_host, int64_t S, int64_t Hq) {
  const auto [B, Hkv, Smax, D] = check_caches(cache_k, cache_v);
  check_bf16_dense(qkv, 2, "qkv");
  TORCH_CHECK(qkv.device() == cache_k.device(), "qkv must be on the caches' device");
  TORCH_CHECK(S >= 1 && S <= Smax && Hq >= 1 && Hq < (1 << 16), "S must be in [1, Smax = ", Smax, "] and Hq positive");
  TORCH_CHECK(qkv.size(0) == B * S && qkv.size(1) == (Hq + 2 * Hkv) * D, "qkv must be [B * S = ", B * S,
              ", (Hq + 2 Hkv) * D = ", (Hq + 2 * Hkv) * D, "], got [", qkv.size(0), ", ", qkv.size(1), "]");
  TORCH_CHECK(qkv.numel() < (1L << 40) && B * S < (1L << 31), "qkv too large");
  const int32_t* h = check_table(start, start_host, B, cache_k, "start");
  for (long b = 0; b < B; ++b)
    TORCH_CHECK(h[b] >= 0 && (long)h[b] + S <= Smax, "start row ", b, ": positions [", h[b], ", + ", S,
                ") leave the cache's ", Smax);
  ++g_decode_launches;
  launch_kv_append(cbf(qkv), bf(cache_k), bf(cache_v), start.data_ptr<int>(), (int)B, (int)S, (int)Hq, (int)Hkv, (int)D,
                   (int)Smax, cur_stream());
}

// q bf16 [B, Hq, D]; row b attends to keys 0 .. lens[b] - 1 of its caches. Returns o bf16 [B, Hq * D].
Tensor decode_attention(Tensor q, Tensor cache_k, Tensor cache_v, Tensor lens, Tensor lens_host, double scale) {
  const auto [B, Hkv, Smax, D] = check_caches(cache_k, cache_v);
  // (q may be the leading columns of the packed projection output: any row stride in whole 16-byte units)
  TORCH_CHECK(q.is_cuda() && q.device() == cache_k.device(), "q must be on the caches' device");
  check_dtype(q, at::kBFloat16, "q");
  check_aligned(q, "q");
  TORCH_CHECK(q.dim() == 3 && q.stride(2) == 1 && q.stride(1) == q.size(2) && q.stride(0) >= q.size(1) * q.size(2) &&
                  q.stride(0) % 8 == 0, "q must be [B, Hq, D] with dense rows and a row stride in whole 16-byte units");
  TORCH_CHECK(D == 64 || D == 128, "decode_attention takes head_dim 64 or 128, got ", D);
  const long Hq = q.size(1);
  TORCH_CHECK(q.size(0) == B && q.size(2) == D && Hq >= 1, "q must be [B = ", B, ", Hq, D = ", D, "]");
  TORCH_CHECK(Hq % Hkv == 0 && Hq / Hkv <= 16, "decode_attention takes Hq % Hkv == 0 and a group of at most 16 "
              "queries, got Hq = ", Hq, ", Hkv = ", Hkv);
  TORCH_CHECK(B <= 65535 && Hkv <= 65535, "decode_attention: too many rows or heads");
  TORCH_CHECK(scale > 0 && scale < 1e6, "scale out of range");
  const int32_t* h = check_table(lens, lens_host, B, cache_k, "lens");
  long longest = 1;
  for (long b = 0; b < B; ++b) {
    TORCH_CHECK(h[b] >= 1 && h[b] <= Smax, "lens row ", b, ": ", h[b], " outside [1, Smax = ", Smax, "]");
    longest = std::max<long>(longest, h[b]);
  }
  const long G = Hq / Hkv, nch = (longest + kDecodeChunk - 1) / kDecodeChunk;
  auto fopt = q.options().dtype(at::kFloat);
  auto ws_ml = torch::empty({B, Hkv, nch, G, 2}, fopt);
  auto ws_o = torch::empty({B, Hkv, nch, G, D}, fopt);
  auto o = torch::empty({B, Hq * D}, q.options());
  ++g_decode_launches;
  launch_decode_attention(cbf(q), q.stride(0), cbf(cache_k), cbf(cache_v), lens.data_ptr<int>(), f32(ws_ml),
                          f32(ws_o), bf(o), (int)B, (int)Hq, (int)Hkv, (int)D, (int)Smax, (int)nch, (float)scale,
                          cur_stream());
  return o;
}

}  // namespace

void bind_decode(pybind11::module_& m) {
  m.def("linear_skinny", &linear_skinny, "x"_a, "w"_a, "y = x . w^T for 1 to 16 rows of x, streaming w once");
  m.def("linear_skinny_ok", [](int64_t M, int64_t N, int64_t K) { return k8s_amd::linear_skinny_ok(M, N, K); }, "M"_a,
        "N"_a, "K"_a, "whether linear_skinny takes the shape");
  m.def("linear_skinny_plan", [](int64_t N, int64_t K) {
    const SkinnyPlan p = k8s_amd::skinny_plan(N, K);
    return std::make_pair(p.kc, p.nsplit);
  }, "N"_a, "K"_a, "(k per chunk, chunks) of linear_skinny's K split");
  m.def("kv_append", &kv_append, "qkv"_a, "cache_k"_a, "cache_v"_a, "start"_a, "start_host"_a, "S"_a, "Hq"_a,
        "copy the k / v columns of a packed projection output into the caches at start[b] + s");
  m.def("decode_attention", &decode_attention, "q"_a, "cache_k"_a, "cache_v"_a, "lens"_a, "lens_host"_a, "scale"_a,
        "one query token per row against the first lens[b] cache positions");
  m.def("decode_launches", [] { return g_decode_launches; }, "decode launcher calls made by this process");
  m.attr("decode_chunk") = k8s_amd::kDecodeChunk;
}

}  // namespace k8s_amd::binding
