// Layer-wise adaptive optimizers on the flat store: LARS (on fused SGD+momentum) and LAMB (on fused Adam).
//
// Both scale each parameter tensor's update by a trust ratio built from two L2 norms over that tensor, so the
// kernels need what optim.hip never did: where one parameter ends and the next begins. The host cuts every
// parameter slot (inside every owned range of a ZeRO-1 shard) into WORK ITEMS of at most kLayerItemMax elements, a
// multiple of 64 each (k8s_amd/ops/optim.py), one row of `items` per piece:
//
//     items[i] = {flat offset, state offset, length, segment}
//
// flat offset indexes master / gradient / bf16 copy, state offset the moment buffers (packed back to back after
// `shard()`), segment is the parameter's index. A step is four launches over that table:
//
//   1. layer_sums    partial[i] = (sum p^2, sum x^2) of item i, one block_sum per item, no atomics.
//                    LARS: x = scaled gradient (a read-only pass). LAMB: the pass also advances and stores m, v and
//                    x = u, the Adam direction plus decay.
//   2. layer_fold    one wave per segment adds its items' partials in item order into sums[segment] (a segment's
//                    items are contiguous in the table). The ZeRO-1 all-reduce of `sums` happens after this.
//   3. layer_ratio   one thread per segment: the trust ratio r, 1 for slots that do not decay or have a zero norm.
//   4. layer_update  LARS: the SGD update with r per item. LAMB: u recomputed from the advanced m, v and the
//                    unchanged p (lamb_u, shared with pass 1; no fp32 scratch copy of u), p -= lr r u. The bf16
//                    working copy of low-precision slots is written in the same pass.
//
// The item -> partial mapping is fixed and no sum depends on the grid size, so a step is bitwise reproducible.
// A zero device clip factor (non-finite gradients) makes every kernel return before its first write: all buffers,
// m / v / sums / ratio included, stay bit-identical. lr and the step come from `hyper` when given (hipGraph replay).
#include "common.h"
#include "launchers.h"

namespace k8s_amd {

namespace {

constexpr int kCols = 4;  // columns of an item row
constexpr uint8_t kDecay = 1, kLowp = 2;  // per-segment flag bits

// LAMB's per-element direction from the advanced moments: both passes call this, so the norm ||u|| of pass 1 is
// the norm of what pass 2 applies. rbc1 = 1 / (1 - b1^t), rbc2 = 1 / (1 - b2^t), w = this slot's weight decay.
__device__ __forceinline__ float lamb_u(float m, float v, float p, float rbc1, float rbc2, float eps, float w) {
  return (m * rbc1) / (sqrtf(v * rbc2) + eps) + w * p;
}

struct Item {
  long off, soff;
  int n4, seg;
};
__device__ __forceinline__ Item load_item(const long* __restrict__ items, int it) {
  const long* e = items + (long)it * kCols;
  Item r;
  r.off = e[0];
  r.soff = e[1];
  r.n4 = (int)(e[2] >> 2);
  r.seg = (int)e[3];
  return r;
}

template <typename GT, bool LAMB>
__global__ void __launch_bounds__(256) layer_sums_kernel(const long* __restrict__ items, int n_items,
                                                         const float* __restrict__ p, float* __restrict__ m1,
                                                         float* __restrict__ m2, const GT* __restrict__ g,
                                                         const uint8_t* __restrict__ flags,
                                                         float* __restrict__ partial, float b1, float b2, float eps,
                                                         float wd, float scale, const float* __restrict__ scale_ptr,
                                                         const float* __restrict__ hyper, float bc1, float bc2) {
  if (scale_ptr && *scale_ptr == 0.f) return;  // non-finite gradients: skipped step, nothing is written
  __shared__ float red[4];
  const float s = scale * (scale_ptr ? *scale_ptr : 1.f);
  if (LAMB && hyper) {
    bc1 = 1.f - powf(b1, hyper[1]);
    bc2 = 1.f - powf(b2, hyper[1]);
  }
  const float rbc1 = 1.f / bc1, rbc2 = 1.f / bc2;
  for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
    const Item e = load_item(items, it);
    const float w = (LAMB && (flags[e.seg] & kDecay)) ? wd : 0.f;
    float sp = 0.f, sx = 0.f;
#pragma unroll 4
    for (int q = threadIdx.x; q < e.n4; q += 256) {
      const long i = e.off + (long)q * 4;
      float gv[4];
      load_grad4<GT>(g, i, gv);
      const float4 pv = *reinterpret_cast<const float4*>(p + i);
      const float* pp = &pv.x;
      if (LAMB) {
        const long k = e.soff + (long)q * 4;
        float4 av = *reinterpret_cast<float4*>(m1 + k);
        float4 bv = *reinterpret_cast<float4*>(m2 + k);
        float* ap = &av.x;
        float* bp = &bv.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float gr = gv[j] * s;
          ap[j] = b1 * ap[j] + (1.f - b1) * gr;
          bp[j] = b2 * bp[j] + (1.f - b2) * gr * gr;
          const float u = lamb_u(ap[j], bp[j], pp[j], rbc1, rbc2, eps, w);
          sp += pp[j] * pp[j];
          sx += u * u;
        }
        *reinterpret_cast<float4*>(m1 + k) = av;
        *reinterpret_cast<float4*>(m2 + k) = bv;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float gr = gv[j] * s;
          sp += pp[j] * pp[j];
          sx += gr * gr;
        }
      }
    }
    sp = block_sum(sp, red);
    sx = block_sum(sx, red);
    if (threadIdx.x == 0) {
      partial[2L * it] = sp;
      partial[2L * it + 1] = sx;
    }
  }
}

// one wave per segment; lane l adds items a+l, a+l+64, ... in order, then the xor butterfly: a fixed order
__global__ void __launch_bounds__(64) layer_fold_kernel(const float* __restrict__ partial,
                                                        const int* __restrict__ seg_start,
                                                        float* __restrict__ sums,
                                                        const float* __restrict__ scale_ptr) {
  if (scale_ptr && *scale_ptr == 0.f) return;
  const int seg = blockIdx.x;
  const int a = seg_start[seg], b = seg_start[seg + 1];
  float sp = 0.f, sx = 0.f;
  for (int i = a + (int)threadIdx.x; i < b; i += 64) {
    sp += partial[2L * i];
    sx += partial[2L * i + 1];
  }
  sp = wave_sum(sp);
  sx = wave_sum(sx);
  if (threadIdx.x == 0) {
    sums[2 * seg] = sp;
    sums[2 * seg + 1] = sx;
  }
}

// LAMB: r = ||p|| / ||u||. LARS: r = eta ||p|| / (||g|| + wd ||p||). 1 where the slot does not decay or a norm is 0.
__global__ void __launch_bounds__(256) layer_ratio_kernel(const float* __restrict__ sums,
                                                          const uint8_t* __restrict__ flags, int n_seg,
                                                          float* __restrict__ ratio, int lamb, float eta, float wd,
                                                          const float* __restrict__ scale_ptr) {
  if (scale_ptr && *scale_ptr == 0.f) return;
  const int seg = blockIdx.x * blockDim.x + threadIdx.x;
  if (seg >= n_seg) return;
  const float pn = sqrtf(sums[2 * seg]), xn = sqrtf(sums[2 * seg + 1]);
  float r = 1.f;
  if ((flags[seg] & kDecay) && pn > 0.f && xn > 0.f) r = lamb ? pn / xn : eta * pn / (xn + wd * pn);
  ratio[seg] = r;
}

template <typename GT, bool LAMB>
__global__ void __launch_bounds__(256) layer_update_kernel(const long* __restrict__ items, int n_items,
                                                           float* __restrict__ p, float* __restrict__ m1,
                                                           const float* __restrict__ m2, const GT* __restrict__ g,
                                                           uint16_t* __restrict__ pbf,
                                                           const uint8_t* __restrict__ flags,
                                                           const float* __restrict__ ratio, float lr, float mu,
                                                           float b1, float b2, float eps, float wd, float scale,
                                                           const float* __restrict__ scale_ptr,
                                                           const float* __restrict__ hyper, float bc1, float bc2,
                                                           int first_step) {
  if (scale_ptr && *scale_ptr == 0.f) return;
  const float s = scale * (scale_ptr ? *scale_ptr : 1.f);
  if (hyper) {
    lr = hyper[0];
    if (LAMB) {
      bc1 = 1.f - powf(b1, hyper[1]);
      bc2 = 1.f - powf(b2, hyper[1]);
    }
  }
  const float rbc1 = 1.f / bc1, rbc2 = 1.f / bc2;
  for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
    const Item e = load_item(items, it);
    const uint8_t f = flags[e.seg];
    const float w = (f & kDecay) ? wd : 0.f;
    const float r = ratio[e.seg];
    const float step = lr * r;
    const bool lowp = pbf && (f & kLowp);
#pragma unroll 4
    for (int q = threadIdx.x; q < e.n4; q += 256) {
      const long i = e.off + (long)q * 4;
      const long k = e.soff + (long)q * 4;
      float4 pv = *reinterpret_cast<float4*>(p + i);
      float4 av = *reinterpret_cast<float4*>(m1 + k);
      float* pp = &pv.x;
      float* ap = &av.x;
      if (LAMB) {
        const float4 bv = *reinterpret_cast<const float4*>(m2 + k);
        const float* bp = &bv.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) pp[j] -= step * lamb_u(ap[j], bp[j], pp[j], rbc1, rbc2, eps, w);
      } else {
        float gv[4];
        load_grad4<GT>(g, i, gv);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float d = r * (gv[j] * s + w * pp[j]);
          const float m = first_step ? d : mu * ap[j] + d;
          ap[j] = m;
          pp[j] -= lr * m;
        }
        *reinterpret_cast<float4*>(m1 + k) = av;
      }
      *reinterpret_cast<float4*>(p + i) = pv;
      if (lowp) store_bf4(pbf, i, pv);
    }
  }
}

int item_grid(int n_items) {
  const long cap = 8L * planner_cus();
  return (int)(n_items < cap ? n_items : cap);
}

}  // namespace

void launch_layer_sums(const long* items, int n_items, const float* p, float* m1, float* m2, const void* g,
                       bool g_bf16, const uint8_t* flags, float* partial, bool lamb, float b1, float b2, float eps,
                       float wd, float scale, const float* scale_ptr, const float* hyper, float bc1, float bc2,
                       hipStream_t st) {
  if (n_items <= 0) return;
  const dim3 grid(item_grid(n_items)), block(256);
#define K8S_LW_SUMS(GT, L)                                                                                       \
  hipLaunchKernelGGL((layer_sums_kernel<GT, L>), grid, block, 0, st, items, n_items, p, m1, m2, (const GT*)g,   \
                     flags, partial, b1, b2, eps, wd, scale, scale_ptr, hyper, bc1, bc2)
  if (lamb) {
    if (g_bf16) K8S_LW_SUMS(uint16_t, true); else K8S_LW_SUMS(float, true);
  } else {
    if (g_bf16) K8S_LW_SUMS(uint16_t, false); else K8S_LW_SUMS(float, false);
  }
#undef K8S_LW_SUMS
}

void launch_layer_fold(const float* partial, const int* seg_start, int n_seg, float* sums, const float* scale_ptr,
                       hipStream_t st) {
  if (n_seg <= 0) return;
  hipLaunchKernelGGL(layer_fold_kernel, dim3(n_seg), dim3(64), 0, st, partial, seg_start, sums, scale_ptr);
}

void launch_layer_ratio(const float* sums, const uint8_t* flags, int n_seg, float* ratio, bool lamb, float eta,
                        float wd, const float* scale_ptr, hipStream_t st) {
  if (n_seg <= 0) return;
  hipLaunchKernelGGL(layer_ratio_kernel, dim3(cdiv(n_seg, 256)), dim3(256), 0, st, sums, flags, n_seg, ratio,
                     (int)lamb, eta, wd, scale_ptr);
}

void launch_layer_update(const long* items, int n_items, float* p, float* m1, const float* m2, const void* g,
                         bool g_bf16, uint16_t* pbf, const uint8_t* flags, const float* ratio, bool lamb, float lr,
                         float mu, float b1, float b2, float eps, float wd, float scale, const float* scale_ptr,
                         const float* hyper, float bc1, float bc2, bool first_step, hipStream_t st) {
  if (n_items <= 0) return;
  const dim3 grid(item_grid(n_items)), block(256);
#define K8S_LW_UPD(GT, L)                                                                                        \
  hipLaunchKernelGGL((layer_update_kernel<GT, L>), grid, block, 0, st, items, n_items, p, m1, m2, (const GT*)g, \
                     pbf, flags, ratio, lr, mu, b1, b2, eps, wd, scale, scale_ptr, hyper, bc1, bc2,             \
                     (int)first_step)
  if (lamb) {
    K8S_LW_UPD(float, true);  // the LAMB update reads no gradient
  } else {
    if (g_bf16) K8S_LW_UPD(uint16_t, false); else K8S_LW_UPD(float, false);
  }
#undef K8S_LW_UPD
}

}  // namespace k8s_amd
