// Stand-alone dropout on the counter generator of rng.h.
//
//  * dropout_kernel: y = keep ? bf16(float(x) * scale) : 0 over row-major [R, D] bf16, 16 B per lane. Forward and
//    backward are the same map (the backward regenerates the mask from the same seed / step / site).
//  * dropout_mask_kernel: the keep bits of rows row0 .. row0 + R - 1, columns 0 .. C - 1 as uint8 -- for tests and
//    debugging; the same two device functions as every fused site.
#include "common.h"
#include "launchers.h"
#include "rng.h"

namespace k8s_amd {

// one 16-B chunk per thread per trip; the rowkey is recomputed per chunk only when the row changes between trips
__global__ void __launch_bounds__(256) dropout_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, long R,
                                                      int D, DropArgs dr) {
  const int nch = D / 8;
  const long total = R * nch;
  const uint64_t seed = (uint64_t)dr.state[0], step = (uint64_t)dr.state[1];
  long last_row = -1;
  uint32_t rk = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long row = i / nch;
    const int ch = (int)(i - row * nch);
    if (row != last_row) {
      rk = philox_rowkey(seed, step, (uint32_t)dr.site, (uint64_t)row);
      last_row = row;
    }
    float v[8];
    load8(x + i * 8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = drop_keep(rk, (uint32_t)(ch * 8 + j), dr.thr) ? v[j] * dr.scale : 0.f;
    store8(y + i * 8, v);
  }
}

__global__ void __launch_bounds__(256) dropout_mask_kernel(uint8_t* __restrict__ out, long row0, long R, int C,
                                                           DropArgs dr) {
  const long total = R * C;
  const uint64_t seed = (uint64_t)dr.state[0], step = (uint64_t)dr.state[1];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / C;
    const int c = (int)(i - r * C);
    const uint32_t rk = philox_rowkey(seed, step, (uint32_t)dr.site, (uint64_t)(row0 + r));
    out[i] = drop_keep(rk, (uint32_t)c, dr.thr) ? 1 : 0;
  }
}

void launch_dropout(const uint16_t* x, uint16_t* y, long R, int D, const DropArgs& dr, hipStream_t st) {
  if (R <= 0 || D <= 0) return;
  hipLaunchKernelGGL(dropout_kernel, dim3(stream_grid(R * (D / 8), 256)), dim3(256), 0, st, x, y, R, D, dr);
}

void launch_dropout_mask(uint8_t* out, long row0, long R, int C, const DropArgs& dr, hipStream_t st) {
  if (R <= 0 || C <= 0) return;
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(stream_grid(R * C, 256)), dim3(256), 0, st, out, row0, R, C, dr);
}

}  // namespace k8s_amd
