// Counter-based dropout mask: a keep bit is a pure function of (seed, step, site, row, col, threshold); nothing is
// stored, and the backward regenerates the forward's bits.
//
//   rowkey = Philox4x32-10(counter = (row lo, row hi, site, step lo), key = (seed lo, seed hi))[0]   (Random123)
//   h      = mix32(rowkey ^ (col * 0x9E3779B1))
//   keep   = h >= thr,  thr = min(floor(p * 2^32 + 0.5), 2^32 - 1)
//
// Philox quality applies once per row (wave-uniform in the norm kernels, two calls per lane in the attention forward, a
// 128-entry LDS table in the one-block attention backward; in the three-kernel attention backward flash_rowkey_kernel
// writes a [B, Hq, Sq] table beside delta, which the dK/dV kernel stages per query tile with lse | delta and the dQ
// kernel reads once per lane); each element then costs ~10 integer VALU operations in whichever axis order the kernel
// holds its elements. ops/reference.py dropout_keep is the same definition in torch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace k8s_amd {

// What a kernel with a dropout site takes: the device int64 [seed, step] pair it reads itself (so a captured graph
// draws a new mask on every replay), the site, the keep threshold and 1 / (1 - thr / 2^32). state == null: off.
struct DropArgs {
  const int64_t* state = nullptr;
  uint32_t thr = 0;
  float scale = 1.f;
  int site = 0;
};

__device__ __forceinline__ uint32_t philox_rowkey(uint64_t seed, uint64_t step, uint32_t site, uint64_t row) {
  uint32_t c0 = (uint32_t)row, c1 = (uint32_t)(row >> 32), c2 = site, c3 = (uint32_t)step;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

__device__ __forceinline__ uint32_t drop_mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ bool drop_keep(uint32_t rowkey, uint32_t col, uint32_t thr) {
  return drop_mix32(rowkey ^ (col * 0x9E3779B1u)) >= thr;
}

// the row's key from a DropArgs (reads the device [seed, step] pair)
__device__ __forceinline__ uint32_t drop_rowkey(const DropArgs& d, uint64_t row) {
  return philox_rowkey((uint64_t)d.state[0], (uint64_t)d.state[1], (uint32_t)d.site, row);
}

}  // namespace k8s_amd
