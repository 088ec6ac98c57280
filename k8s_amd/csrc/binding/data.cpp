// Dataset entry points of k8s_amd._C: the fused augmentation kernel (kernels/augment.hip).
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

}  // namespace

void bind_data(pybind11::module_& m) {
  m.def("augment", &augment, "src"_a, "table"_a, "a"_a, "b"_a, "S"_a, "layout"_a,
        "gather + crop / resize + flip + normalise a uint8 batch into the stem's bf16 input");
  m.def("augment_launches", [] { return g_augment_launches; }, "augment kernels launched by this process");
}

}  // namespace k8s_amd::binding
