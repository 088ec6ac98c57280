// Fused backward of the 1x1 convolution that opens a ResNet identity bottleneck (conv1: 4w -> w channels, w = 64 at
// 56x56 and w = 128 at 28x28), with the backward apply pass of the BatchNorm + ReLU behind it (bn1) formed on load.
// bwd1x1_fused.hip is the mirror case (conv3: the wide side is the gradient); here the narrow side is the gradient and
// the wide side the input. One pass over row tiles gives, with N = 4w,
//
//   dx1[m][k] = bf16(fma(sc, relu_on(x1) ? dz1 : 0, fma(B, x1, D)))       bn_bwd_apply_kernel's expression, never stored
//   dx[m][n]  = bf16(float(bf16(sum_k dx1[m][k] w[k][n])) + (abit ? dy[m][n] : 0))   gemm_short's masked-addend epilogue
//   sums[.][0][n] += sum_m g,  sums[.][1][n] += sum_m g (x3[m][n] - mean[n]),  g = bit ? stored dx : 0   (its EPI 3)
//   dW[k][n] (+)= sum_m dx1[m][k] xin[m][n]                                 fp32
//
// where today bn_bwd_apply writes dx1 [M][w] and gemm_short (data gradient) and wgrad_stream (weight gradient) each
// read it back and stream a wide [M][4w] tensor past it: 26.5 GB against 22.8 GB at batch 3072 / 56x56.
//
//  * Persistent grid, one 512-thread workgroup per CU (planner_cus()), walking 32-row tiles pair + i * npairs. A
//    workgroup owns 256 columns of dx / dW: N = 512 runs as two workgroups per row tile, placed on one XCD and adjacent
//    in dispatch order (bwd1x1_fused.hip's placement), so the narrow tiles they share come from HBM once; both form dx1.
//  * A stage is [dz1 | x1 | xin | dy | x3 | addend bits | ReLU bits] = 58 KB (w = 64) or 66 KB (w = 128), every operand
//    by LDS-DMA into a ring of two with raw barriers. With two slots no younger stage is in flight when stage s is
//    waited for -- stage s + 1 is issued after the barrier that follows the wait -- so the wait is vmcnt(0) in every
//    iteration (bwd1x1_fused.hip, ONLOAD); the dx stores of stage s - 1 are behind the dW products by then. Nothing
//    loads through VGPRs inside the loop. Every tile is a workgroup-uniform 64-bit base plus a 32-bit lane offset.
//  * The narrow images are [32 rows][128 B] per 64 channels (swz128: read row-wise by the dx product, transposed by the
//    dW product), the xin image [32][512 B] with swz_g (transposed reads), the dy and x3 images [32][512 B] with the
//    16-B unit XOR (row & 15), which is also the layout of the bf16 product tile the dx MFMAs leave: the element pass
//    then reads all three lane-linearly, a thread's two units (rows r, r + 16) hold the same channels, and its 16-B
//    stores cover whole 512-B row segments.
//  * dx1 is formed in place over the dz1 image (thread = one 16-B unit, its 4 x 8 table constants in registers).
//  * dx: wave v keeps w[:, 32 columns] as MFMA A fragments for the whole walk; the products accumulate in gemm_short's
//    order (one v_mfma_f32_16x16x32_bf16 per 32-deep chunk, chunks ascending), so dx is that kernel's bit for bit.
//  * dW: wave v owns 32 columns x w rows in accumulators across the walk, both operands read transposed
//    (ds_read_b64_tr_b16), one 32-row K step per tile. It leaves as one fp32 [w][N] slab per row-tile walker, summed
//    in walker order by slab_reduce_kernel (no atomics: the weight gradient stays repeatable bit for bit).
//  * Rows past M read the tile's last valid row (clamped offsets); the transform writes zero dx1 rows for them, which
//    add nothing to dW, and the element pass stores nothing and takes no sums for them.
//  * The two-BatchNorm sums (gemm_short's EPI 4: the previous block is a stage-entry block) are not built: a third
//    wide image per stage does not fit beside a two-slot ring at w = 128 (2 x 82 KB). Those layers keep their route.
#include <algorithm>
#include <stdexcept>

#include "common.h"
#include "launchers.h"
#include "lds_image.h"

namespace k8s_amd {
namespace c1f {

constexpr int THREADS = 512;
constexpr int RS = 32;    // rows per tile
constexpr int NC = 256;   // columns of dx / dW per workgroup
constexpr int REPL = kConvStatReplicas;

typedef __attribute__((ext_vector_type(4))) int int4_t;

// (the images are bwd1x1_fused.hip's: lds_image.h holds their swizzles and the transposed fragment read)
struct Args {
  const uint16_t *dz1, *x1;  // [M][W]: bn1's incoming gradient and input
  const float* params;       // bn1's [sc | B | D | shift], fp32 [4][W]
  const uint16_t* w;         // [W][N]
  const uint16_t* xin;       // [M][N]: the convolution's input
  const uint16_t* dy;        // [M][N]: the residual addend
  const uint8_t* abits;      // [M][N / 8]: its packed bits
  const uint16_t* x3;        // [M][N]: the input of the BatchNorm whose sums are taken
  const uint8_t* bits;       // [M][N / 8]: that BatchNorm's packed ReLU bits
  const float* mean;         // [N]
  uint16_t* dx;              // [M][N]
  float* sums;               // [REPL][2][N]
  float* dwpart;             // fp32 [walker][W][N]
  int M, ntiles, npairs;
};

//   <64>: 2 x 58 KB ring + 16 KB product tile;  <128>: 2 x 66 KB ring + 16 KB
template <int W>
__global__ void __launch_bounds__(THREADS, 1) conv1_fused_kernel(Args a) {
  constexpr int N = 4 * W, HALVES = N / NC, KC = W / 32, NJ = W / 16;
  constexpr int IMG_N = RS * W * 2;   // a narrow image: W / 64 half-images of [32][128 B]
  constexpr int IMG_W = RS * NC * 2;  // a wide image: [32][512 B]
  constexpr int OFF_Z = 0, OFF_X1 = IMG_N, OFF_XIN = 2 * IMG_N, OFF_DY = OFF_XIN + IMG_W, OFF_X3 = OFF_DY + IMG_W;
  constexpr int OFF_AB = OFF_X3 + IMG_W, OFF_BT = OFF_AB + 1024, STAGE = OFF_BT + 1024;
  constexpr int NT = RS * W / 8;  // 16-B units of a narrow tile: the threads of the transform
  static_assert(NT % 64 == 0 && NT <= THREADS && RS * NC / 8 == 2 * THREADS && RS * NC / 8 == 1024, "tile");
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE + IMG_W];
  static_assert(sizeof(smem) <= 160 * 1024, "LDS");
  static_assert(THREADS * 64 <= 2 * STAGE, "sums partials reuse the ring");
  char* stg = smem + 2 * STAGE;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bid = blockIdx.x;
  int pair = bid, chalf = 0;
  if constexpr (HALVES == 2) {  // the two halves of a pair: one XCD, adjacent in dispatch order
    const int slot = bid >> 3;
    chalf = slot & 1;
    pair = (slot >> 1) * 8 + (bid & 7);
  }
  const int c0 = chalf * NC;
  const int n = pair < a.ntiles ? (a.ntiles - pair + a.npairs - 1) / a.npairs : 0;
  if (n == 0) return;
  const long M = a.M;

  // ---- w fragments of this wave's 32 columns: A operand of dx^T = w^T dx1^T (row = column n, k = 8 (l >> 4) + j)
  int4_t wf[2][KC];
  {
    const uint16_t* wp = a.w + (long)(8 * (lane >> 4)) * N + c0 + wid * 32 + (lane & 15);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
        bf16x8_t v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (short)wp[(long)(kc * 32 + j) * N + nb * 16];
        wf[nb][kc] = __builtin_bit_cast(int4_t, v);
      }
  }
  // ---- the transform's unit: half-image tid >> 8, row (tid >> 3) & 31, unit tid & 7 holds channels tc .. tc + 7
  const int trow = (tid >> 3) & 31;
  const int tc = (tid >> 8) * 64 + (((tid & 7) ^ swz128(trow)) << 3);
  float tsc[8], tB[8], tD[8], tsh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const bool act = tid < NT;
    tsc[j] = act ? a.params[tc + j] : 0.f;
    tB[j] = act ? a.params[W + tc + j] : 0.f;
    tD[j] = act ? a.params[2 * W + tc + j] : 0.f;
    tsh[j] = act ? a.params[3 * W + tc + j] : 0.f;
  }
  // ---- the element pass's units: rows (tid >> 5) and + 16, position tid & 31 holds columns c0 + 8 eu .. + 7
  const int erow = tid >> 5, eup = tid & 31, eu = eup ^ erow;
  float mu[8], ps[8], pq[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = a.mean[c0 + eu * 8 + j];
    ps[j] = pq[j] = 0.f;
  }
  // every ordinary load is consumed here, before the first LDS-DMA is issued
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) asm volatile("" : "+v"(wf[nb][kc]));
#pragma unroll
  for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(tsc[j]), "+v"(tB[j]), "+v"(tD[j]), "+v"(tsh[j]), "+v"(mu[j]));

  auto issue = [&](int slot, int i) {
    char* st = smem + slot * STAGE;
    const long m0 = (long)(pair + i * a.npairs) * RS;
    const unsigned last = (unsigned)min((long)RS - 1, M - 1 - m0);  // rows past M read the last valid row
    if (wid < NT / 64) {
      const unsigned off = min((unsigned)trow, last) * W + tc;
      glds16(a.dz1 + m0 * W + off, st + OFF_Z + wid * 1024);
      glds16(a.x1 + m0 * W + off, st + OFF_X1 + wid * 1024);
    }
    const uint16_t* xb = a.xin + m0 * N + c0;
    const uint16_t* db = a.dy + m0 * N + c0;
    const uint16_t* x3b = a.x3 + m0 * N + c0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const unsigned row = j * 16 + erow;
      const unsigned ro = min(row, last) * N;
      glds16(xb + ro + ((eup ^ swz_g(row)) << 3), st + OFF_XIN + j * (THREADS * 16) + wid * 1024);
      glds16(db + ro + (eu << 3), st + OFF_DY + j * (THREADS * 16) + wid * 1024);
      glds16(x3b + ro + (eu << 3), st + OFF_X3 + j * (THREADS * 16) + wid * 1024);
    }
    if (wid >= THREADS / 64 - 2) {  // the two bit tiles, 32 B a row: lane = 16 B of row lane >> 1
      const unsigned off = min((unsigned)lane >> 1, last) * (N / 8) + chalf * (NC / 8) + (lane & 1) * 16;
      if (wid == THREADS / 64 - 2) glds16(a.abits + m0 * (N / 8) + off, st + OFF_AB);
      else glds16(a.bits + m0 * (N / 8) + off, st + OFF_BT);
    }
  };

  f32x4_t dwa[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) dwa[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  issue(0, 0);
  int slot = 0;
  for (int s = 0; s < n; ++s) {
    // stage s landed: no younger stage is in flight (two slots), so the wait is vmcnt(0) whatever a wave's load count
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();  // every wave's share of stage s is in LDS; stage s-1's reads are done
    if (s + 1 < n) issue(slot ^ 1, s + 1);
    char* S = smem + slot * STAGE;
    const int last = (int)min((long)RS - 1, M - 1 - (long)(pair + s * a.npairs) * RS);

    // ---- dx1 = bf16(fma(sc, relu_on(x1) ? dz1 : 0, fma(B, x1, D))) over the dz1 image, unit by unit (the expression
    // and rounding of bn_bwd_apply_kernel); rows past M become zero rows
    if (tid < NT) {
      char* zp = S + OFF_Z + tid * 16;
      const bf16x8_t gv = *reinterpret_cast<const bf16x8_t*>(zp);
      const bf16x8_t xv = *reinterpret_cast<const bf16x8_t*>(zp + IMG_N);
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xf = bf2f((uint16_t)xv[j]);
        const float g = relu_on(xf, tsc[j], tsh[j]) ? bf2f((uint16_t)gv[j]) : 0.f;
        o[j] = __builtin_fmaf(tsc[j], g, __builtin_fmaf(tB[j], xf, tD[j]));
        o[j] = trow <= last ? o[j] : 0.f;
      }
      *reinterpret_cast<bf16x8_t*>(zp) = pack_bf16x8(o);
    }
    lds_barrier();  // the dx1 tile is complete

    // ---- dx product: columns wid * 32 .., all 32 rows; lane holds row (l & 15), columns 4 (l >> 4) + r
    {
      f32x4_t acc[2][2];
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
        const int u = kc * 4 + (lane >> 4);
        const char* img = S + OFF_Z + (u >> 3) * (RS * 128);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
          const int row = mb * 16 + (lane & 15);
          const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(img + row * 128 + (((u & 7) ^ swz128(row)) << 4));
#pragma unroll
          for (int nb = 0; nb < 2; ++nb)
            acc[mb][nb] = mfma16(__builtin_bit_cast(mfma_bf16x8, wf[nb][kc]), __builtin_bit_cast(mfma_bf16x8, b),
                                 acc[mb][nb]);
        }
      }
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          const int row = mb * 16 + (lane & 15);
          const int unit = wid * 4 + nb * 2 + (lane >> 5), half = (lane >> 4) & 1;
          bf16x4_t o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = (short)f2bf(acc[mb][nb][r]);
          *reinterpret_cast<bf16x4_t*>(stg + row * 512 + ((unit ^ (row & 15)) << 4) + half * 8) = o;
        }
    }
    lds_barrier();  // the product tile is complete

    // ---- element pass: dx = bf16(product + (abit ? dy : 0)), stored; g = bit ? dx : 0 into the sums -- the roundings
    // and the sums of gemm_short's masked-addend epilogue (rows past M: no store, no sums)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = j * 16 + erow;
      const int off = j * (THREADS * 16) + tid * 16;
      const bf16x8_t pv = *reinterpret_cast<const bf16x8_t*>(stg + off);
      const bf16x8_t dv = *reinterpret_cast<const bf16x8_t*>(S + OFF_DY + off);
      const bf16x8_t xv = *reinterpret_cast<const bf16x8_t*>(S + OFF_X3 + off);
      const uint32_t keep = *reinterpret_cast<const uint8_t*>(S + OFF_AB + row * 32 + eu);
      const uint32_t bits = row <= last ? (uint32_t) * reinterpret_cast<const uint8_t*>(S + OFF_BT + row * 32 + eu) : 0u;
      float o[8];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        o[i] = bf2f((uint16_t)pv[i]) + (((keep >> i) & 1u) ? bf2f((uint16_t)dv[i]) : 0.f);
      const bf16x8_t ov = pack_bf16x8(o);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float g = (bits >> i) & 1u ? bf2f((uint16_t)ov[i]) : 0.f;
        ps[i] += g;
        pq[i] = __builtin_fmaf(g, bf2f((uint16_t)xv[i]) - mu[i], pq[i]);
      }
      if (row <= last)
        *reinterpret_cast<bf16x8_t*>(a.dx + ((long)(pair + s * a.npairs) * RS + row) * N + c0 + eu * 8) = ov;
    }

    // ---- dW: columns wid * 32 .. of dW x all W rows, one 32-row K step
    {
      TrRaw ar[2], br[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        tr_load<128, swz128>(br[j], S + OFF_Z + (j >> 2) * (RS * 128), (j & 3) * 16, 0, lane);
#pragma unroll
      for (int i = 0; i < 2; ++i) tr_load<512, swz_g>(ar[i], S + OFF_XIN, wid * 32 + i * 16, 0, lane);
#pragma unroll
      for (int j = 0; j < NJ; j += 4)
        K8S_LDS_TIE8("s_waitcnt lgkmcnt(0)", br[j].lo, br[j].hi, br[j + 1].lo, br[j + 1].hi, br[j + 2].lo, br[j + 2].hi,
                     br[j + 3].lo, br[j + 3].hi);
      K8S_LDS_TIE4("s_waitcnt lgkmcnt(0)", ar[0].lo, ar[0].hi, ar[1].lo, ar[1].hi);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          dwa[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(join8(ar[i].lo, ar[i].hi), join8(br[j].lo, br[j].hi),
                                                              dwa[i][j], 0, 0, 0);
    }
    slot ^= 1;
  }

  // ---- dW partials: lane holds dW[k = j * 16 + (lane & 15)][c0 + wid * 32 + i * 16 + 4 (lane >> 4) + r]. The walker's
  // slab, plain 16-B stores: the slabs are summed in walker order by slab_reduce_kernel, so dW does not depend on the order
  // the workgroups finish in
  {
    float* slab = a.dwpart + (long)pair * W * N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        *reinterpret_cast<f32x4_t*>(slab + (long)(j * 16 + (lane & 15)) * N + c0 + wid * 32 + i * 16 +
                                    4 * (lane >> 4)) = dwa[i][j];
  }
  // ---- sums: the 16 threads of a column unit fold through LDS, one atomic per (column, sum) per workgroup
  __syncthreads();
  float* part = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    part[tid * 16 + j] = ps[j];
    part[tid * 16 + 8 + j] = pq[j];
  }
  __syncthreads();
  {
    const int col = tid & (NC - 1), which = tid / NC;
    const int u = col >> 3, r = col & 7;
    float v = 0.f;
#pragma unroll 4
    for (int row = 0; row < 16; ++row) v += part[(row * 32 + (u ^ row)) * 16 + which * 8 + r];
    atomicAdd(a.sums + (long)(bid % REPL) * 2 * N + (long)which * N + c0 + col, v);
  }
}

// dw[i] (+)= sum_z slab[z][i], the slabs in a fixed order whatever order the walkers finished in (the splitk_reduce
// idiom), with fp64 partial sums: 8 interleaved groups of slabs, then the groups in order. One rounding to fp32 at the
// end -- a serial fp32 sum of 256 slabs measured 3.4x the streaming weight gradient's error against fp64 at M = 9600 --
// and 8 x the threads of a thread per element, for a product this small (W N = 16k or 64k elements).
__global__ void __launch_bounds__(256) slab_reduce_kernel(const float* __restrict__ ws, int nslab, long mn,
                                                          float* __restrict__ out, int accumulate) {
  __shared__ double red[256];
  const int e = threadIdx.x & 31, g = threadIdx.x >> 5;
  const long i = (long)blockIdx.x * 32 + e;  // mn % 32 == 0
  double acc = 0.0;
#pragma unroll 4
  for (int z = g; z < nslab; z += 8) acc += (double)ws[(long)z * mn + i];
  red[threadIdx.x] = acc;
  __syncthreads();
  if (g == 0) {
    double t = accumulate ? (double)out[i] : 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += red[k * 32 + e];
    out[i] = (float)t;
  }
}

// row-tile walkers (pairs of workgroups at N = 512) of a launch
static int walkers(int N) {
  const int cus = std::max(1, planner_cus());
  return N == NC ? cus : std::max(16, cus / 16 * 16) / 2;
}

}  // namespace c1f

// The contract: (W, N) = (64, 256) or (128, 512), 1 <= M < 2^31.
bool conv1_fused_ok(long M, int W, int N) {
  return M >= 1 && M < (1L << 31) && ((W == 64 && N == 256) || (W == 128 && N == 512));
}
// fp32 elements of Conv1Fused::dw_partials: one [W][N] slab per walker that has a tile
long conv1_fused_workspace(long M, int W, int N) {
  return std::min<long>(c1f::walkers(N), (M + c1f::RS - 1) / c1f::RS) * W * N;
}

void launch_conv1_fused(const Conv1Fused& c, long M, int W, int N, bool accumulate, hipStream_t st) {
  using namespace c1f;
  if (!conv1_fused_ok(M, W, N)) throw std::runtime_error("conv1_fused: (W, N) = (64, 256) or (128, 512), M < 2^31");
  if (!(c.dz1 && c.x1 && c.params && c.w && c.xin && c.dy && c.abits && c.x3 && c.bits && c.mean && c.dx && c.sums &&
        c.dw && c.dw_partials))
    throw std::runtime_error("conv1_fused: every operand is required");
  Args a{c.dz1, c.x1, c.params, c.w, c.xin, c.dy, c.abits, c.x3, c.bits, c.mean, c.dx, c.sums, c.dw_partials,
         (int)M, (int)((M + RS - 1) / RS), walkers(N)};
  if (W == 64) hipLaunchKernelGGL((conv1_fused_kernel<64>), dim3(a.npairs), dim3(THREADS), 0, st, a);
  else hipLaunchKernelGGL((conv1_fused_kernel<128>), dim3(2 * a.npairs), dim3(THREADS), 0, st, a);
  // walkers 0 .. min(npairs, ntiles) - 1 each wrote a slab: dw (+)= their sum, in that order
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(W * N / 32), dim3(256), 0, st, c.dw_partials,
                     std::min(a.npairs, a.ntiles), (long)W * N, c.dw, accumulate ? 1 : 0);
}

}  // namespace k8s_amd
