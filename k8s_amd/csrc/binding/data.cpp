// Dataset entry points of k8s_amd._C: the fused augmentation kernel (kernels/augment.hip) and the token batch kernels
// (kernels/token_batch.hip).
#include <string>

#include "binding/common.h"

namespace k8s_amd::binding {
namespace {

long g_augment_launches = 0;  // kernel launches so far: the tests check that a rejected call never got this far

// src uint8 [M, Hs, Ws, 3] on the GPU; table int32 [N, 6] on the host, rows (src index, y0, x0, h, w, flip); a, b: the
// three fp32 normalisation pairs. The table is validated here, row by row, before anything is allocated or launched;
// then it is uploaded and the kernel (which clamps every coordinate once more) runs on the current stream.
Tensor augment(Tensor src, Tensor table, std::vector<double> a, std::vector<double> b, int64_t S,
               const std::string& layout) {
  check_cuda(src, "src");
  check_dtype(src, at::kByte, "src");
  TORCH_CHECK(src.dim() == 4 && src.size(3) == 3 && src.size(0) >= 1 && src.size(1) >= 1 && src.size(2) >= 1,
              "src must be uint8 [M, Hs, Ws, 3]");
  TORCH_CHECK(table.device().is_cpu(), "table must be a CPU tensor (it is validated on the host, then uploaded)");
  check_dtype(table, at::kInt, "table");
  TORCH_CHECK(table.dim() == 2 && table.size(1) == 6 && table.size(0) >= 1 && table.is_contiguous(),
              "table must be a contiguous int32 [N, 6]");
  TORCH_CHECK(a.size() == 3 && b.size() == 3, "a and b must have 3 values each");
  const bool s2d = layout == "s2d";
  TORCH_CHECK(s2d || layout == "nhwc8", "layout must be \"nhwc8\" or \"s2d\", not \"", layout, "\"");
  TORCH_CHECK(S >= 1 && S <= 65536 && !(s2d && S % 2), "S must be positive (and even for the s2d layout), got ", S);
  const long M = src.size(0), Hs = src.size(1), Ws = src.size(2), N = table.size(0);
  TORCH_CHECK(M < (1L << 31) && Hs < (1L << 24) && Ws < (1L << 24), "src too large");
  const long Ho = S / 2 + 3, total = s2d ? N * Ho * Ho : N * S * S;
  TORCH_CHECK(total < (1L << 31), "augment: too many output pixels in one call");
  const int32_t* t = table.data_ptr<int32_t>();
  for (long n = 0; n < N; ++n, t += 6) {
    const long idx = t[0], y0 = t[1], x0 = t[2], h = t[3], w = t[4], flip = t[5];
    TORCH_CHECK(idx >= 0 && idx < M, "table row ", n, ": source index ", idx, " outside [0, ", M, ")");
    TORCH_CHECK(h >= 1 && w >= 1, "table row ", n, ": box ", h, " x ", w, " must be at least 1 x 1");
    TORCH_CHECK(flip == 0 || flip == 1, "table row ", n, ": flip must be 0 or 1, got ", flip);
    if (h != S || w != S) {
      TORCH_CHECK(y0 >= 0 && x0 >= 0 && y0 + h <= Hs && x0 + w <= Ws, "table row ", n, ": resized box (", y0, ", ", x0,
                  ", ", h, ", ", w, ") leaves the ", Hs, " x ", Ws, " source");
    } else {  // a copy row may hang over the edge (zero padding), by less than 2^24 so its coordinates stay exact
      TORCH_CHECK(y0 > -(1L << 24) && y0 < (1L << 24) && x0 > -(1L << 24) && x0 < (1L << 24), "table row ", n,
                  ": offset out of range");
    }
  }
  k8s_amd::AugNorm nm;
  for (int c = 0; c < 3; ++c) {
    nm.a[c] = (float)a[c];
    nm.b[c] = (float)b[c];
  }
  // through pinned memory, asynchronously: a pageable upload would make the host wait for the stream to drain, once
  // per batch, and the next step's launches would no longer run ahead of the GPU
  auto dtable = table.pin_memory().to(src.device(), /*non_blocking=*/true);
  auto out = s2d ? torch::empty({N, Ho, Ho, 16}, src.options().dtype(at::kBFloat16))
                 : torch::empty({N, S, S, 8}, src.options().dtype(at::kBFloat16));
  ++g_augment_launches;
  launch_augment(src.data_ptr<uint8_t>(), dtable.data_ptr<int32_t>(), (int)N, (int)M, (int)Hs, (int)Ws, (int)S, nm, s2d,
                 bf(out), cur_stream());
  return out;
}

long g_token_launches = 0;  // mlm_batch + causal_batch kernel launches, counted like g_augment_launches

// The token array of a split: int32, or uint16 data passed as an int16 view (read unsigned). Returns true for uint16.
bool check_token_src(const Tensor& src) {
  check_cuda(src, "src");
  TORCH_CHECK(src.scalar_type() == at::kInt || src.scalar_type() == at::kShort,
              "src has dtype ", src.scalar_type(), ", expected int32 or (uint16 data viewed as) int16");
  TORCH_CHECK(src.dim() == 1 && src.size(0) >= 1, "src must be a 1-D token array");
  return src.scalar_type() == at::kShort;
}

void check_host_i64(const Tensor& t, int64_t cols, const char* name) {
  TORCH_CHECK(t.device().is_cpu(), name, " must be a CPU tensor (it is validated on the host, then uploaded)");
  check_dtype(t, at::kLong, name);
  TORCH_CHECK(t.is_contiguous() && t.size(0) >= 1 && (cols ? t.dim() == 2 && t.size(1) == cols : t.dim() == 1), name,
              " must be a contiguous int64 [N", cols ? ", 6]" : "]");
}

// src: the tokens on the GPU; table int64 [N, 6] on the host, rows (a0, la, b0, lb, n, ord); special (pad, cls, sep,
// mask). Every row is validated here before anything is allocated or launched; then the table is uploaded through
// pinned memory and the kernel (which clamps once more) runs on the current stream.
bool check_mlm_args(const Tensor& src, const Tensor& table, int64_t S, int64_t P, int64_t vocab,
                    const std::vector<int64_t>& special, int64_t stream) {
  const bool u16 = check_token_src(src);
  TORCH_CHECK(vocab >= 2 && vocab <= 0x7fffffffLL, "vocab must be in [2, 2^31 - 1], got ", vocab);
  TORCH_CHECK(!u16 || vocab <= 65536, "uint16 tokens need vocab <= 65536, got ", vocab);
  check_host_i64(table, 6, "table");
  TORCH_CHECK(S >= 1 && S <= 512, "S must be in [1, 512], got ", S);
  TORCH_CHECK(P >= 1 && P <= S, "P must be in [1, S], got ", P);
  TORCH_CHECK(stream >= 0 && stream < (1 << 20), "stream out of range");
  TORCH_CHECK(special.size() == 4, "special must be (pad, cls, sep, mask)");
  for (int64_t v : special) TORCH_CHECK(v >= 0 && v < vocab, "special id ", v, " outside [0, vocab = ", vocab, ")");
  const int64_t T = src.size(0), N = table.size(0);
  TORCH_CHECK(N < (1L << 22), "mlm_batch: too many rows in one call");
  const int64_t* t = table.data_ptr<int64_t>();
  for (int64_t r = 0; r < N; ++r, t += 6) {
    const int64_t a0 = t[0], la = t[1], b0 = t[2], lb = t[3], n = t[4], ord = t[5];
    TORCH_CHECK(la >= 1 && lb >= 1 && la <= S && lb <= S && la + lb + 3 <= S, "table row ", r, ": lengths ", la, " + ",
                lb, " + 3 must fit S = ", S, " with both segments non-empty");
    TORCH_CHECK(a0 >= 0 && a0 <= T - la && b0 >= 0 && b0 <= T - lb, "table row ", r, ": a segment leaves the ", T,
                " tokens of src");
    TORCH_CHECK(n >= 1 && n <= P && n <= la + lb, "table row ", r, ": n = ", n, " must be in [1, min(P, la + lb)]");
    TORCH_CHECK(ord >= 0, "table row ", r, ": negative ordinal");
  }
  return u16;
}

std::vector<Tensor> mlm_batch(Tensor src, Tensor table, int64_t S, int64_t P, int64_t vocab,
                              std::vector<int64_t> special, int64_t seed, int64_t stream) {
  const bool u16 = check_mlm_args(src, table, S, P, vocab, special, stream);
  const int64_t T = src.size(0), N = table.size(0);
  const k8s_amd::TokSpecial sp{(int)special[0], (int)special[1], (int)special[2], (int)special[3]};
  auto dtable = table.pin_memory().to(src.device(), /*non_blocking=*/true);
  auto opt = src.options().dtype(at::kLong);
  auto ids = torch::empty({N, S}, opt), types = torch::empty({N, S}, opt);
  auto labels = torch::empty({N, P}, opt), positions = torch::empty({N, P}, opt);
  ++g_token_launches;
  launch_mlm_batch(src.data_ptr(), u16, T, dtable.data_ptr<int64_t>(), (int)N, (int)S, (int)P, (uint32_t)vocab, sp,
                   (uint64_t)seed, (int)stream, ids.data_ptr<int64_t>(), types.data_ptr<int64_t>(),
                   labels.data_ptr<int64_t>(), positions.data_ptr<int64_t>(), cur_stream());
  return {ids, types, labels, positions};
}

// mlm_batch without padding: the N samples back to back in one stream of T rows. cu int64 [N + 1] on the host, the
// samples' first rows: cu[0] = 0 and cu[n + 1] - cu[n] = la + lb + 3 of table row n; T is cu[N] rounded up to a
// multiple of 128. Everything mlm_batch validates is validated, then cu and T, all before anything is allocated or
// launched. Returns ids, token_types, pos (int64 [T]), labels, rows (int64 [N, P]), cls_rows (int64 [N]) and the span
// bounds lo, hi (int32 [1, T]).
std::vector<Tensor> mlm_batch_unpadded(Tensor src, Tensor table, Tensor cu, int64_t T, int64_t S, int64_t P,
                                       int64_t vocab, std::vector<int64_t> special, int64_t seed, int64_t stream) {
  const bool u16 = check_mlm_args(src, table, S, P, vocab, special, stream);
  const int64_t Tn = src.size(0), N = table.size(0);
  TORCH_CHECK(cu.device().is_cpu(), "cu must be a CPU tensor (it is validated on the host, then uploaded)");
  check_dtype(cu, at::kLong, "cu");
  TORCH_CHECK(cu.dim() == 1 && cu.is_contiguous() && cu.size(0) == N + 1, "cu must be a contiguous int64 [N + 1] with "
              "N = ", N, " table rows");
  const int64_t* c = cu.data_ptr<int64_t>();
  const int64_t* t = table.data_ptr<int64_t>();
  TORCH_CHECK(c[0] == 0, "cu[0] must be 0, got ", c[0]);
  for (int64_t r = 0; r < N; ++r)
    TORCH_CHECK(c[r + 1] - c[r] == t[6 * r + 1] + t[6 * r + 3] + 3, "cu row ", r, ": ", c[r + 1], " - ", c[r],
                " is not la + lb + 3 = ", t[6 * r + 1] + t[6 * r + 3] + 3);
  TORCH_CHECK(T >= c[N], "T = ", T, " is below cu[N] = ", c[N]);
  TORCH_CHECK(T % 128 == 0, "T = ", T, " must be a multiple of 128");
  TORCH_CHECK(T - c[N] < 128, "T = ", T, " must be cu[N] = ", c[N], " rounded up to a multiple of 128");
  TORCH_CHECK(T < (1L << 31), "mlm_batch_unpadded: too many stream rows in one call");
  const k8s_amd::TokSpecial sp{(int)special[0], (int)special[1], (int)special[2], (int)special[3]};
  auto both = torch::cat({table.reshape({-1}), cu});  // one upload: [6 N | N + 1]
  auto dboth = both.pin_memory().to(src.device(), /*non_blocking=*/true);
  auto opt = src.options().dtype(at::kLong), opt32 = src.options().dtype(at::kInt);
  auto ids = torch::empty({T}, opt), types = torch::empty({T}, opt), pos = torch::empty({T}, opt);
  auto labels = torch::empty({N, P}, opt), rows = torch::empty({N, P}, opt), cls_rows = torch::empty({N}, opt);
  auto lo = torch::empty({1, T}, opt32), hi = torch::empty({1, T}, opt32);
  ++g_token_launches;
  launch_mlm_batch_unpadded(src.data_ptr(), u16, Tn, dboth.data_ptr<int64_t>(), dboth.data_ptr<int64_t>() + 6 * N, T,
                            (int)N, (int)S, (int)P, (uint32_t)vocab, sp, (uint64_t)seed, (int)stream,
                            ids.data_ptr<int64_t>(), types.data_ptr<int64_t>(), pos.data_ptr<int64_t>(),
                            labels.data_ptr<int64_t>(), rows.data_ptr<int64_t>(), cls_rows.data_ptr<int64_t>(),
                            lo.data_ptr<int>(), hi.data_ptr<int>(), cur_stream());
  return {ids, types, pos, labels, rows, cls_rows, lo, hi};
}

// starts int64 [N] on the host: ids = src[start : start + S], labels = src[start + 1 : start + S + 1].
std::vector<Tensor> causal_batch(Tensor src, Tensor starts, int64_t S) {
  const bool u16 = check_token_src(src);
  check_host_i64(starts, 0, "starts");
  const int64_t T = src.size(0), N = starts.size(0);
  TORCH_CHECK(S >= 1 && S < (1L << 24) && N * S < (1L << 31), "causal_batch: S or N * S out of range");
  const int64_t* s = starts.data_ptr<int64_t>();
  for (int64_t r = 0; r < N; ++r)
    TORCH_CHECK(s[r] >= 0 && s[r] <= T - S - 1, "starts row ", r, ": window [", s[r], ", + ", S, " + 1) leaves the ", T,
                " tokens of src");
  auto dstarts = starts.pin_memory().to(src.device(), /*non_blocking=*/true);
  auto opt = src.options().dtype(at::kLong);
  auto ids = torch::empty({N, S}, opt), labels = torch::empty({N, S}, opt);
  ++g_token_launches;
  launch_causal_batch(src.data_ptr(), u16, T, dstarts.data_ptr<int64_t>(), (int)N, (int)S, ids.data_ptr<int64_t>(),
                      labels.data_ptr<int64_t>(), cur_stream());
  return {ids, labels};
}

// causal_batch with document boundaries. starts index src (the rebased offsets of a streamed batch), abs_starts are the
// same windows' positions in the split, both int64 [N] on the host; doc_tok int64 [D + 1] on the GPU, the documents'
// token offsets (checked by the caller when it uploaded them: the host never reads device data here); split_tokens is
// their last entry, the split's length. Returns ids, labels (int64) and lo, hi, pos (int32), all [N, S].
std::vector<Tensor> causal_doc_batch(Tensor src, Tensor starts, Tensor abs_starts, Tensor doc_tok, int64_t S,
                                     int64_t split_tokens) {
  const bool u16 = check_token_src(src);
  check_host_i64(starts, 0, "starts");
  check_host_i64(abs_starts, 0, "abs_starts");
  const int64_t T = src.size(0), N = starts.size(0);
  TORCH_CHECK(abs_starts.size(0) == N, "starts and abs_starts must have the same length");
  check_cuda(doc_tok, "doc_tok");
  check_dtype(doc_tok, at::kLong, "doc_tok");
  TORCH_CHECK(doc_tok.dim() == 1 && doc_tok.size(0) >= 2 && doc_tok.size(0) < (1L << 31) && doc_tok.is_contiguous() &&
                  doc_tok.device() == src.device(), "doc_tok must be a contiguous int64 [D + 1] on src's device");
  TORCH_CHECK(S >= 1 && S < (1L << 24) && N * S < (1L << 31), "causal_doc_batch: S or N * S out of range");
  const int64_t* s = starts.data_ptr<int64_t>();
  const int64_t* ab = abs_starts.data_ptr<int64_t>();
  for (int64_t r = 0; r < N; ++r) {
    TORCH_CHECK(s[r] >= 0 && s[r] <= T - S - 1, "starts row ", r, ": window [", s[r], ", + ", S, " + 1) leaves the ", T,
                " tokens of src");
    TORCH_CHECK(ab[r] >= 0 && ab[r] <= split_tokens - S - 1, "abs_starts row ", r, ": window [", ab[r], ", + ", S,
                " + 1) leaves the ", split_tokens, " tokens of the split");
  }
  auto both = torch::stack({starts, abs_starts}).contiguous();  // one upload: [2, N]
  auto dboth = both.pin_memory().to(src.device(), /*non_blocking=*/true);
  auto opt = src.options().dtype(at::kLong), opt32 = src.options().dtype(at::kInt);
  auto ids = torch::empty({N, S}, opt), labels = torch::empty({N, S}, opt);
  auto lo = torch::empty({N, S}, opt32), hi = torch::empty({N, S}, opt32), pos = torch::empty({N, S}, opt32);
  ++g_token_launches;
  launch_causal_doc_batch(src.data_ptr(), u16, T, dboth.data_ptr<int64_t>(), dboth.data_ptr<int64_t>() + N,
                          doc_tok.data_ptr<int64_t>(), doc_tok.size(0) - 1, (int)N, (int)S, ids.data_ptr<int64_t>(),
                          labels.data_ptr<int64_t>(), lo.data_ptr<int>(), hi.data_ptr<int>(), pos.data_ptr<int>(),
                          cur_stream());
  return {ids, labels, lo, hi, pos};
}

}  // namespace

void bind_data(pybind11::module_& m) {
  m.def("causal_doc_batch", &causal_doc_batch, "src"_a, "starts"_a, "abs_starts"_a, "doc_tok"_a, "S"_a,
        "split_tokens"_a, "gather causal-LM windows with their document bounds, positions and boundary-aware labels");
  m.def("mlm_batch", &mlm_batch, "src"_a, "table"_a, "S"_a, "P"_a, "vocab"_a, "special"_a, "seed"_a, "stream"_a = 0,
        "assemble a BERT pretraining batch (ids, token types, MLM labels and positions) from a token array");
  m.def("mlm_batch_unpadded", &mlm_batch_unpadded, "src"_a, "table"_a, "cu"_a, "T"_a, "S"_a, "P"_a, "vocab"_a,
        "special"_a, "seed"_a, "stream"_a = 0,
        "assemble a BERT pretraining batch as one unpadded token stream with its span bounds and gather rows");
  m.def("causal_batch", &causal_batch, "src"_a, "starts"_a, "S"_a, "gather causal-LM windows (ids, shifted labels)");
  m.def("token_launches", [] { return g_token_launches; }, "token batch kernels launched by this process");
  m.def("augment", &augment, "src"_a, "table"_a, "a"_a, "b"_a, "S"_a, "layout"_a,
        "gather + crop / resize + flip + normalise a uint8 batch into the stem's bf16 input");
  m.def("augment_launches", [] { return g_augment_launches; }, "augment kernels launched by this process");
}

}  // namespace k8s_amd::binding
