// Shared by the Python bindings of the k8s_amd gfx950 kernels (module k8s_amd._C, one binding file per kernel family).
//
// Every entry point validates device, dtype, contiguity and shape on the host before launching, so a mis-shaped call
// raises a Python exception instead of faulting the GPU: validate everything, then allocate, then launch. The checks
// that more than one entry point needs are the named ones below. Kernels are launched on PyTorch's current HIP stream
// so they compose with torch ops, streams and hipGraph capture.
#pragma once

#include <torch/extension.h>

#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <vector>

#include "kernels/launchers.h"

namespace k8s_amd::binding {

using at::Tensor;
using OptTensor = c10::optional<Tensor>;
using namespace pybind11::literals;  // "name"_a in the registrations

inline hipStream_t cur_stream() { return at::hip::getCurrentHIPStream().stream(); }

inline uint16_t* bf(const Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }
inline const uint16_t* cbf(const Tensor& t) { return reinterpret_cast<const uint16_t*>(t.data_ptr()); }
inline float* f32(const Tensor& t) { return t.data_ptr<float>(); }
inline const float* optf(const OptTensor& t) { return t.has_value() ? t->data_ptr<float>() : nullptr; }

// ------------------------------------------------------------------ checks
inline void check_cuda(const Tensor& t, const char* name) {  // GPU and contiguous
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}
inline void check_dtype(const Tensor& t, at::ScalarType d, const char* name) {
  TORCH_CHECK(t.scalar_type() == d, name, " has dtype ", t.scalar_type(), ", expected ", d);
}
inline void check_aligned(const Tensor& t, const char* name) {
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0, name, " must be 16-byte aligned");
}
inline void check_bf16(const Tensor& t, const char* name) {
  check_cuda(t, name);
  check_dtype(t, at::kBFloat16, name);
}
// check_bf16, 16-byte aligned and of rank `ndim` (-1: any)
inline void check_bf16_dense(const Tensor& t, int ndim, const char* name) {
  check_bf16(t, name);
  TORCH_CHECK(ndim < 0 || t.dim() == ndim, name, " must have ", ndim, " dimensions");
  check_aligned(t, name);
}
// GPU, contiguous fp32 vector of C elements: per channel (gamma / beta / mean / invstd / running statistics / their
// gradients) or a flat buffer
inline void check_channel_f32(const Tensor& t, long C, const char* name) {
  check_cuda(t, name);
  check_dtype(t, at::kFloat, name);
  TORCH_CHECK(t.numel() == C, name, " must have ", C, " fp32 elements, has ", t.numel());
}
// statistics buffer fp32 [R, 2, C] (GPU, contiguous): `exact` R = conv_stat_replicas (what the producing epilogues
// index), else whatever R its size holds. Returns R.
inline int check_stat_sums(const Tensor& t, long C, const char* name, bool exact) {
  check_cuda(t, name);
  check_dtype(t, at::kFloat, name);
  TORCH_CHECK(C > 0, name, ": no channels");
  TORCH_CHECK(exact ? t.numel() == (long)kConvStatReplicas * 2 * C : t.numel() % (2 * C) == 0, name,
              " must be fp32 [", exact ? "conv_stat_replicas" : "R", ", 2, ", C, "]");
  return (int)(t.numel() / (2 * C));
}
// packed one-bit mask: GPU, uint8, contiguous, one bit per element (bit j of byte e = element 8e + j)
inline const uint8_t* check_bit_mask(const Tensor& t, long elements, const char* name) {
  check_cuda(t, name);
  check_dtype(t, at::kByte, name);
  TORCH_CHECK(t.numel() * 8 == elements, name, " must be packed uint8, one bit for each of ", elements, " elements");
  return t.data_ptr<uint8_t>();
}
// optional fp32 [2 * C] BatchNorm (scale | shift) of a normalize-on-load operand; nullptr when absent
inline const float* xform_ptr(const OptTensor& xf, long C) {
  if (!xf || !xf->defined()) return nullptr;
  check_channel_f32(*xf, 2 * C, "xform (BatchNorm scale | shift)");
  TORCH_CHECK(C % 8 == 0, "xform channels must be a multiple of 8");
  return xf->data_ptr<float>();
}
// dropout arguments (rng.h). state: device int64 [seed, step], read by the kernels themselves (never by the host);
// thr / scale: the keep threshold and 1 / (1 - thr / 2^32) (ops/reference.py drop_params); site: the call site's
// small integer
inline DropArgs drop_args(const Tensor& state, int64_t thr, double scale, int64_t site) {
  check_cuda(state, "dropout state"); check_dtype(state, at::kLong, "dropout state");
  TORCH_CHECK(state.numel() >= 2, "dropout state must be an int64 [seed, step] tensor");
  TORCH_CHECK(thr > 0 && thr <= 0xffffffffLL, "dropout threshold out of range (p must be in (0, 1))");
  TORCH_CHECK(site >= 0 && site <= 0x7fffffffLL, "dropout site out of range");
  DropArgs d;
  d.state = state.data_ptr<int64_t>();
  d.thr = (uint32_t)thr;
  d.scale = (float)scale;
  d.site = (int)site;
  return d;
}

// ------------------------------------------------------------------ 256 x 256 GEMM routing and scratch (gemm.cpp)
// K8S_AMD_GEMM256=0 routes every product to the 128 x 128 kernel, =2 every product the 256 x 256 kernel can take
// (A/B comparisons, debugging); read per call, so one process can A/B both kernels
int gemm256_mode();
bool use_gemm256(long M, long N, long K, bool a_kmajor, bool b_kmajor);
// Zero-initialised int words for the stream-K tickets / flags, one buffer per (device, stream) and process
int* sk_sync_words(long n, const c10::Device& dev);
// The stream-K tail of a partial-wave 256 x 256 grid: fp32 partial slabs (caching allocator, stream-ordered) on
// `like`'s device and the self-resetting ticket / flag words; both null when the plan has no tail.
struct SkScratch {
  SkScratch(const Gemm256Plan& plan, const Tensor& like);
  float* slab_ptr() const { return sync ? slabs.data_ptr<float>() : nullptr; }
  int* sync_ptr() const { return sync; }
 private:
  Tensor slabs;
  int* sync = nullptr;
};

// ------------------------------------------------------------------ BatchNorm-backward sums of a dgrad epilogue
// What BnBwdSums and GemmShortBnStats share. x: the BatchNorm's input, bf16 with C channels last; mean fp32 [C]; sums
// zeroed fp32 [conv_stat_replicas, 2, C]. Returns C.
template <class B>
long fill_x_mean_sums(B& b, const Tensor& x, const Tensor& mean, const Tensor& sums) {
  check_bf16_dense(x, -1, "bn x");
  TORCH_CHECK(x.dim() >= 1, "bn x: channels last");
  const long C = x.size(-1);
  check_channel_f32(mean, C, "bn mean");
  check_stat_sums(sums, C, "bn sums", true);
  b.x = cbf(x);
  b.mean = f32(mean);
  b.sums = f32(sums);
  return C;
}
// mask kind: the BatchNorm's stored packed ReLU bits, optionally with a second BatchNorm fed by the same gradient
template <class B>
void fill_mask_kind(B& b, const Tensor& x, const Tensor& mask, const Tensor& mean, const Tensor& sums,
                    const OptTensor& x2, const OptTensor& mean2, const OptTensor& sums2) {
  const long C = fill_x_mean_sums(b, x, mean, sums);
  b.mask = check_bit_mask(mask, x.numel(), "bn mask");
  if (!x2) return;
  TORCH_CHECK(mean2 && sums2, "x2 needs mean2 and sums2");
  check_bf16_dense(*x2, -1, "bn x2");
  TORCH_CHECK(x2->sizes() == x.sizes(), "x2: the shape of x");
  check_channel_f32(*mean2, C, "bn mean2");
  check_stat_sums(*sums2, C, "bn sums2", true);
  b.x2 = cbf(*x2);
  b.mean2 = f32(*mean2);
  b.sums2 = f32(*sums2);
}
// relu kind (no mask): gamma / beta / invstd give the forward's ReLU decision; else the mask kind
inline BnBwdSums bn_bwd_sums(const Tensor& x, const Tensor& mean, const Tensor& sums, const OptTensor& mask,
                             const OptTensor& gamma, const OptTensor& beta, const OptTensor& invstd,
                             const OptTensor& x2, const OptTensor& mean2, const OptTensor& sums2) {
  BnBwdSums b;
  if (mask) {
    TORCH_CHECK(!gamma && !beta && !invstd, "bn sums: packed mask or gamma / beta / invstd, not both");
    fill_mask_kind(b, x, *mask, mean, sums, x2, mean2, sums2);
    return b;
  }
  TORCH_CHECK(gamma && beta && invstd && !x2 && !mean2 && !sums2, "bn sums (relu kind): gamma / beta / invstd, one BN");
  const long C = fill_x_mean_sums(b, x, mean, sums);
  check_channel_f32(*gamma, C, "bn gamma"); check_channel_f32(*beta, C, "bn beta");
  check_channel_f32(*invstd, C, "bn invstd");
  b.gamma = f32(*gamma);
  b.beta = f32(*beta);
  b.invstd = f32(*invstd);
  return b;
}
// the mask kind for the short-K streaming GEMM's epilogue
inline GemmShortBnStats gemm_short_bn_stats(const Tensor& x, const Tensor& mask, const Tensor& mean,
                                            const Tensor& sums, const OptTensor& x2, const OptTensor& mean2,
                                            const OptTensor& sums2) {
  GemmShortBnStats b;
  fill_mask_kind(b, x, mask, mean, sums, x2, mean2, sums2);
  return b;
}

// ------------------------------------------------------------------ one per family file
using Module = pybind11::module_;
void bind_optim(Module&), bind_batchnorm(Module&), bind_norm(Module&), bind_gemm(Module&), bind_conv(Module&);
void bind_attention(Module&), bind_elementwise(Module&), bind_data(Module&), bind_decode(Module&);

}  // namespace k8s_amd::binding
