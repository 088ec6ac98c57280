// LDS images read transposed (ds_read_b64_tr_b16): the swizzles, the fragment read and the waits shared by the kernels
// that stage [rows (m)][RB bytes] tiles with global_load_lds and read them as MFMA operands with the reduction along
// the rows (bwd1x1_fused.hip, conv1_fused.hip, wgrad_stream.hip). One level above mfma.h's tr16_asm / join8 /
// K8S_LDS_TIE8.
//
//  * A swizzle maps a row to the XOR applied to the index of a 16-B unit inside that row, on the per-lane SOURCE
//    address of the fill and again on the read:
//      swz128  128-B rows (64 channels): conflict-free both row-wise (ds_read_b128) and transposed
//      swz256  256-B rows (128 channels), transposed reads (mfma.h's mn_swz)
//      swz_g   512-B or wider rows read both ways: the 16 rows of a ds_read_b128 lane group get 16 distinct units
#pragma once
#include "mfma.h"

namespace k8s_amd {

__device__ __forceinline__ int swz128(int r) { return 2 * (((r >> 1) & 1) | (((r >> 3) & 1) << 1)); }
__device__ __forceinline__ int swz256(int r) { return 2 * ((r & 3) | (((r >> 3) & 1) << 2)); }
__device__ __forceinline__ int swz_g(int r) { return (2 * ((r & 3) | (((r >> 3) & 1) << 2))) | ((r >> 2) & 1); }

// Transposed fragment of a [rows (m)][RB bytes] image swizzled by SWZ: lane l holds column rb + (l & 15), rows
// kk*32 + 8*(l >> 4) + j (kk: the 32-row block; an image of 32 rows passes 0). Issued as inline asm (tr16_asm: the
// builtin would make hipcc drain the LDS-DMA ring before every read); ready after a K8S_LDS_TIE* wait that names it.
struct TrRaw {
  short4_t lo, hi;
};
template <int RB, int (*SWZ)(int)>
__device__ __forceinline__ void tr_load(TrRaw& r, const char* img, int rb, int kk, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int u = (rb >> 3) + (p >> 1);
  const int r0 = kk * 32 + 8 * g + q, r1 = r0 + 4;
  const int u0 = u ^ SWZ(r0), u1 = u ^ SWZ(r1);
  tr16_asm(r.lo, img + r0 * RB + (u0 << 4) + (p & 1) * 8);
  tr16_asm(r.hi, img + r1 * RB + (u1 << 4) + (p & 1) * 8);
}
// K8S_LDS_TIE8 for four registers
#define K8S_LDS_TIE4(w, a, b, c, d) asm volatile(w : "+v"(a), "+v"(b), "+v"(c), "+v"(d))

// workgroup barrier after this wave's own LDS reads and writes have completed (LDS-DMA fills are counted in vmcnt: the
// caller waits for those itself); the compiler moves no memory access across it
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

}  // namespace k8s_amd
