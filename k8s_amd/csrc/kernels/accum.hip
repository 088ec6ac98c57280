// Gradient accumulation on the flat gradient buffer (parallel/accum.py): two element-wise fp32 streaming passes over a
// 64-aligned range of two equally laid out flat buffers.
//
//   grad_accumulate: acc[i] = first ? g[i] : acc[i] + g[i]   after every micro-batch but the last. `first` makes the
//                    pass a copy, so the accumulation buffer is never zero-filled (8 B/element instead of 12).
//   grad_fold:       g[i] = g[i] + acc[i]                     on the last micro-batch, bucket by bucket, right before a
//                    bucket's collective; optionally also writes bf16(g[i]) (round to nearest even, as cast_bf16) so the
//                    bf16 transport needs no cast pass of its own (14 B/element instead of 12 + 6).
//
// Both are dst = dst + src (or dst = src) with a fixed operand order, one fp32 add per element: the result does not
// depend on the grid, an accumulated gradient is a fixed-order sum and LARS / LAMB stay bitwise reproducible.
//
// One kernel, three forms. 16-B accesses, U independent vectors in flight per thread and operand, a grid from
// stream_grid (planner_cus) with a grid-stride loop, 64-bit indices (Llama-3-8B's store has 8.03e9 elements); no
// atomics, no LDS, no scratch. A block works on U consecutive runs of 256 vectors per trip (a 16 KB span per operand):
// with the grid capped at 8 blocks per CU this layout measured 5.2 TB/s on the 110 M-element BERT-base store where the
// layout of sumsq_kernel (a thread's U vectors a whole grid apart) measured 3.7, and 5.2 against 4.7 on 1.5 G elements.
#include "common.h"
#include "launchers.h"

namespace k8s_amd {

namespace {
constexpr int kAccumUnroll = 4;
constexpr int kAccumBlock = 256;

__device__ __forceinline__ float4 add4(const float4& a, const float4& b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
}  // namespace

// dst = FIRST ? src : dst + src, and with BF also out_bf = bf16(dst). n4: float4 vectors in the range (a multiple of
// 16); dst / src / out_bf already point at its first element.
template <bool FIRST, bool BF>
__global__ void __launch_bounds__(kAccumBlock) grad_accum_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                                 uint16_t* __restrict__ out_bf, long n4) {
  constexpr int U = kAccumUnroll;
  constexpr long kChunk = (long)kAccumBlock * U;  // vectors per block and trip
  float4* __restrict__ dp = reinterpret_cast<float4*>(dst);
  const float4* __restrict__ sp = reinterpret_cast<const float4*>(src);
  const long trip = (long)gridDim.x * kChunk;
  long chunk = (long)blockIdx.x * kChunk;  // first vector of this block's chunk
  for (; chunk + kChunk <= n4; chunk += trip) {
    const long q = chunk + threadIdx.x;
    float4 sv[U], dv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) sv[u] = sp[q + u * kAccumBlock];
    if (!FIRST) {
#pragma unroll
      for (int u = 0; u < U; ++u) dv[u] = dp[q + u * kAccumBlock];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float4 v = FIRST ? sv[u] : add4(dv[u], sv[u]);
      dp[q + u * kAccumBlock] = v;
      if (BF) store_bf4(out_bf, 4 * (q + u * kAccumBlock), v);
    }
  }
  if (chunk < n4) {  // the range's ragged last chunk: one block, one vector per thread and trip
    for (long q = chunk + threadIdx.x; q < n4; q += kAccumBlock) {
      const float4 v = FIRST ? sp[q] : add4(dp[q], sp[q]);
      dp[q] = v;
      if (BF) store_bf4(out_bf, 4 * q, v);
    }
  }
}

// ---------------------------------------------------------------- launchers
// n: elements in the range, a multiple of 64 (checked by the binding); n == 0 launches nothing
template <bool FIRST, bool BF>
static void launch_accum(float* dst, const float* src, uint16_t* out_bf, long n, hipStream_t st) {
  if (n <= 0) return;
  const long n4 = n / 4;
  const int grid = stream_grid((n4 + kAccumUnroll - 1) / kAccumUnroll, kAccumBlock);  // one chunk per block and trip
  hipLaunchKernelGGL((grad_accum_kernel<FIRST, BF>), dim3(grid), dim3(kAccumBlock), 0, st, dst, src, out_bf, n4);
}

void launch_grad_accumulate(float* acc, const float* g, long n, bool first, hipStream_t st) {
  if (first)
    launch_accum<true, false>(acc, g, nullptr, n, st);
  else
    launch_accum<false, false>(acc, g, nullptr, n, st);
}

void launch_grad_fold(float* g, const float* acc, uint16_t* out_bf, long n, hipStream_t st) {
  if (out_bf)
    launch_accum<false, true>(g, acc, out_bf, n, st);
  else
    launch_accum<false, false>(g, acc, nullptr, n, st);
}

}  // namespace k8s_amd
