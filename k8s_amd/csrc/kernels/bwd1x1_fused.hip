// K2 fused backward of a 1x1 convolution whose input BatchNorm + ReLU is normalised on load (ResNet-50's conv3 at
// 56x56 and 28x28: C = 64 -> K = 256 and C = 128 -> K = 512). One pass over gy [M][K] and x [M][C] gives
//
//   dz[m][c]  = sum_k gy[m][k] w[k][c]                               bf16, rounded once
//   dW[k][c] (+)= sum_m gy[m][k] z[m][c],  z = bf16(relu(fma(x, scale, shift)))   fp32 (gemm.hip XForm rounding)
//   sums[.][0][c] += sum_m g,  sums[.][1][c] += sum_m g (x - mean),  g = relu_on(x) ? stored dz : 0
//
// where the weight gradient (gemm.hip, xform_b) followed by the data gradient with the BatchNorm-backward sums
// (gemm_dgrad_bnstats) read gy and x twice: 13.6 GB against 7.4 GB at batch 3072 / 56x56, the wide tensor being gy.
//
//  * Persistent grid, one 512-thread workgroup per CU (planner_cus()), walking row tiles pair + i * npairs. A
//    workgroup owns 64 channels: C = 128 runs as two workgroups per row tile (the products and the sums are
//    independent per channel), placed on one XCD (bid % 8) and adjacent in dispatch order so that the gy tile they
//    share comes from HBM once and from L2 after (wgrad_stream.hip places its tiles the same way).
//  * A stage is RS rows of gy (K-major, 16-B units XOR-swizzled by swz_g(row)) and of x (128-B rows, swz128), filled by
//    global_load_lds into a ring of NSLOT stages with counted vmcnt waits and raw barriers; rows past M are
//    zero-filled from a zero line (the transposed reads need EXEC all ones, and a zero gy row makes its dz, its share
//    of dW and of the sums zero whatever relu(shift) the x row becomes).
//  * dz: w never enters LDS. Wave (rh, ct) keeps the fragments of w[:, 16 channels] in registers for the whole walk
//    (K / 32 x 4 VGPRs) as the MFMA's A operand and reads its rows of the gy tile K-major with ds_read_b128; the
//    result lands as 4 channels x 1 row per lane, goes to a bf16 staging tile, and leaves in full 128-B rows.
//  * One element pass per stage (thread = one 16-B unit, fixed channels for the whole walk): reads the staged dz and
//    the raw x unit, stores dz, adds the sums in registers, and overwrites the x unit in place with z.
//  * dW: wave w owns K / 8 rows of dW x 64 channels in accumulators across the walk; both operands are read
//    transposed (ds_read_b64_tr_b16) from the same gy image and the z image, as in wgrad_stream.hip. The partials
//    leave once per workgroup through fp32 atomics (16 MB chip-wide at K = 256, 32 MB at K = 512).
//  * swz_g serves both read patterns of the gy image: the 16 rows of a ds_read_b128 lane group get 16 distinct units
//    of a 256-B bank row, and the 8 rows of a transposed read's 32-lane group (r..r+3, r+8..r+11) 8 distinct 32-B pairs.
//    Measured (rocprofv3 --pmc, batch 3072): SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.39 at K = 256 and 0.37 at
//    K = 512 over the whole kernel -- more than the fragment reads' layout predicts; the 8-B staging writes of dz and
//    the element pass have not been looked at separately.
//
// ONLOAD (launch_bwd1x1_fused with a Bwd1x1Bn3): gy is not stored anywhere. It is dx3, the gradient the residual
// BatchNorm after the convolution (bn3) would have written, dx3 = bf16(fma(sc, mask ? dy : 0, fma(B, x3, D))) -- the
// expression, nesting and rounding helper of bn_bwd_apply_kernel -- and the kernel forms it tile by tile from that
// BatchNorm's incoming dy, its input x3, its packed ReLU mask and its [sc | B | D] table, which is complete before
// this kernel starts. The apply pass (read dy, x3, mask; write dx3) and this kernel's read of dx3 go away: 22.5 GB ->
// 12.6 GB at batch 3072 / 56x56.
//  * A stage is [dy image | x3 image | mask rows | x image]: the x3 image has the dy image's layout (same swizzle, same
//    lane -> unit map), the mask tile is RS * K / 8 contiguous bytes, one or two waves' 16-B loads. That is 74 KB
//    (K = 256) or 70 KB (K = 512) a stage, so the ring has two slots.
//  * vmcnt: with two slots no younger stage is in flight when stage s is waited for -- stage s + 1 is issued after
//    the barrier that follows the wait, into the slot stage s - 1's dW reads have just left -- so the wait is
//    vmcnt(0) in every iteration, whatever a wave's load count per stage (2 LG, +1 for the mask waves, +1 for the x
//    waves), and the dz stores of stage s - 1, long issued, cost it nothing. Nothing else loads through VGPRs inside
//    the loop. The loads of stage s + 1 then have all of stage s (transform, dz, element pass, dW) to land.
//  * After that barrier every thread rewrites its LG 16-B units of the dy image in place (it reads the dy unit, the x3
//    unit at the same offset and the mask byte of (row, unit)), and one more barrier separates the pass from the dz
//    MFMAs and the transposed dW reads. Everything after the tile is the plain form's code.
//  * The table: at K = 256 a thread's units lie 16 rows apart, which swz_g maps to the same channel group, so its
//    3 x 8 constants stay in registers; at K = 512 they lie 8 rows apart (two groups), w's fragments and the dW
//    accumulators hold 128 VGPRs, and the table sits in LDS (fp32 [3K], read four channels at a time).
//  * Rows past M: the plain form's zero line would turn into fma(B, x3, D) != 0 here, so this form reads the tile's
//    last valid row in their place (which also makes every load a workgroup-uniform base plus a 32-bit lane offset:
//    the per-lane 64-bit addresses and the zero-line select did not fit in the registers left at K = 512) and the
//    transform writes zeros for them: the zero gy rows the rest of the kernel relies on.
//  * At K = 512 both workgroups of a pair transform the whole tile (duplicated VALU / LDS work); measured per layer
//    (benchmarks/bn3_onload.py) the form still beats apply + plain there, by less than at K = 256.
//
// FINAL (launch_bwd1x1_fused with a Bwd1x1Final; (C, K) = (64, 256) only): the x side of a convolution that reads a
// stored tensor and whose data gradient is the second into it -- ResNet's stage-1 downsample convolution on the stem
// pool's output, after conv1's. Per row m and channel c
//   dW uses x as stored (no xform; the x image is not rewritten);
//   out[m][c] = bf16(float(bf16(product)) + float(addend[m][c])), written over the addend: the two roundings of the
//   tile kernel's accumulating epilogue (gemm.hip: "the staged value is already bf16"), whose launch this one
//   replaces, so the step computes what it computed (a single rounding of the fp32 sum was built first: it differed
//   from that kernel in 26 % of the elements by one ulp, enough to move the stem's dbeta -- a sum that cancels -- by
//   1.4e-2 in a batch-2 block, tests/test_dual_onload_gpu.py's bound being 1e-2);
//   g = bit ? stored out : 0, sums[0] += g, sums[1] += g (xw - mean): the pool kind (winner x [M][64], its packed ReLU
//   bits [M][8]) of gemm_dgrad_bnstats_mask without add_src.
// Both the plain and the ONLOAD form exist (gy a materialised gradient, or dy transformed on load exactly as above).
//  * Space: the addend, the winner x and the bits are 16.5 KB per 64-row tile more, which the ONLOAD <256, 64, 2, 1>
//    ring (156 of 160 KB) has no room for. The final forms therefore walk 32-row tiles: a stage is [dy | x3 | mask | x
//    | addend | winner x | bits] = 16 + 16 + 1 + 4 + 4 + 4 + 1 KB = 46 KB in a ring of three (plain: 16 + 4 + 4 + 4 + 1
//    = 29 KB, ring of four), every operand by LDS-DMA, so "nothing loads through VGPRs inside the loop" still holds
//    and there is no second kind of load to count. Both forms use the RS = 32 dz path, so their fp32 sums have one
//    order and out agrees bit for bit between them.
//  * Loads per stage and wave: LG (plain, 2) or 2 LG (ONLOAD, 4) for every wave; +1 for the ONLOAD mask wave (0); +3
//    for the element-pass waves 0..3 (x, addend, winner x: same lane -> unit map, same swz128 image); +1 for wave 7's
//    bits, 4 B per lane (global_load_lds_dword: row lane / 2, half lane & 1 -- 64 lanes are exactly the tile's 256 B,
//    and an 8-B row can be clamped or zero-filled per lane, which a 16-B unit spanning two rows could not be).
//  * vmcnt: the ring logic is the plain form's, now also for ONLOAD. When stage s is waited for, the younger stages in
//    flight are s + 1 (.. s + NSLOT - 2), each at least LPS = LG or 2 LG loads of this wave, so vmcnt(younger * LPS)
//    retires all of stage s: a wave with extra loads in a younger stage (up to 4 + 1 + 3 of them on wave 0) only waits
//    for the first of those too, which were issued a whole stage earlier. The out stores are older than every load
//    counted and change nothing. The loads are in order and of one kind, as before.
//  * The element pass reads the staged dz unit, the addend unit, the winner x unit and one bits byte, adds, rounds,
//    stores out, and adds the sums over the stored values; x is left alone.
//  * Rows past M: zero rows of gy give dz = 0, but out = addend would not be zero where the ONLOAD form's clamped
//    loads repeat the last valid row, so both forms store nothing and take no sums for them (bits read as 0).
//  * dW leaves as one fp32 [K][64] slab per workgroup (plain stores, 16 MB chip-wide -- what the other forms send
//    through atomics) and splitk_reduce sums the slabs in workgroup order: the layer's weight gradient was
//    wgrad_stream's, which is repeatable bit for bit, and tests/test_resnet_gpu.py compares whole-model gradients of
//    two runs for equality. No memset of dW.
//  * In place: a tile's addend rows are in LDS (its stage has been waited for) before the same workgroup stores its
//    out rows, and no other workgroup touches them.
#include <algorithm>
#include <stdexcept>

#include "common.h"
#include "launchers.h"
#include "lds_image.h"

namespace k8s_amd {
namespace b1f {

constexpr int THREADS = 512;
constexpr int CT = 64;  // channels per workgroup

__device__ __attribute__((aligned(64))) uint16_t g_zero16[64];

typedef __attribute__((ext_vector_type(4))) int int4_t;

struct Args {
  const uint16_t *gy, *x, *w;  // ONLOAD: gy is dy, and the tile becomes dx3 from the next three
  const uint16_t* x3;
  const uint8_t* mask;
  const float* params;
  const float *xform, *gamma, *beta, *mean, *invstd;
  uint16_t* dz;
  float* dw;
  float* sums;
  int M, C, ntiles, npairs;
  // FINAL: dz is the addend's own storage (out = bf16(bf16 product + addend), in place), xw / bits the pooled
  // forward's winner x [M][64] and its packed ReLU bits [M][8], mean the winner's BatchNorm mean
  const uint16_t *addend, *xw;
  const uint8_t* bits;
  float* dwpart;  // FINAL: fp32 [workgroup][K][C] partials of dW, summed in workgroup order after the kernel
};

// 4 B per lane into LDS at (wave-uniform base + lane * 4): the FINAL form's bits tile, 8-B rows
__device__ __forceinline__ void glds4(const void* src, void* lds_base) {
  __builtin_amdgcn_global_load_lds(src, (lds_void*)lds_base, 4, 0, 0);
}

//   <256, 64, 3, 1>: 3 x 40 KB ring + 8 KB staging;  <512, 32, 4, 2>: 4 x 36 KB ring + 4 KB staging
//   ONLOAD <256, 64, 2, 1>: 2 x 74 KB ring + 8 KB;   <512, 32, 2, 2>: 2 x 70 KB ring + 4 KB + 7.25 KB of tables
//   FINAL  <256, 32, 4, 1>: 4 x 29 KB ring + 4 KB;   ONLOAD FINAL <256, 32, 3, 1>: 3 x 46 KB ring + 4 KB
template <int K, int RS, int NSLOT, int HALVES, bool ONLOAD, bool FINAL = false>
__global__ void __launch_bounds__(THREADS, 1) bwd1x1_fused_kernel(Args a) {
  constexpr int RB = K * 2, UG = K / 8;
  constexpr int IMG_G = RS * RB, IMG_X = RS * 128;
  constexpr int IMG_M = ONLOAD ? RS * UG : 0;  // packed mask rows: UG bytes each
  constexpr int OFF_X = IMG_G + (ONLOAD ? IMG_G + IMG_M : 0);  // [gy | x3 | mask | x]
  // FINAL: [.. | x | addend | winner x | bits]; the bits tile is RS * 8 B, one wave's 4-B loads, in a 1-KB slot
  constexpr int OFF_A = OFF_X + IMG_X, OFF_W = OFF_A + IMG_X, OFF_B = OFF_W + IMG_X;
  constexpr int STAGE = FINAL ? OFF_B + 1024 : OFF_X + IMG_X, RING = NSLOT * STAGE;
  static_assert(!FINAL || (K == 256 && RS == 32 && HALVES == 1), "the final form: (C, K) = (64, 256), 32-row tiles");
  constexpr int LG = RS * UG / THREADS;  // gy LDS-DMA per thread per stage
  constexpr int LPS = ONLOAD ? 2 * LG : LG;  // ... and the LDS-DMA every wave issues per stage
  // dx3's per-channel constants (sc | B | D): a thread's logical unit is the same for all its LG units when the rows
  // j * THREADS / UG apart agree in the bits swz_g reads (K = 256) -- registers; else an fp32 [3K] table in LDS
  constexpr bool TREG = ONLOAD && (THREADS / UG) % 16 == 0;
  constexpr bool TLDS = ONLOAD && !TREG;
  static_assert(!ONLOAD || (IMG_M % 1024 == 0 && IMG_M / 1024 <= THREADS / 64), "mask tile: whole 1-KB wave loads");
  constexpr int XT = RS * 8;             // 16-B units of an x tile: the threads of the element pass
  constexpr int NKS = K / 32, KW = K / 8, KTW = KW / 16;
  static_assert(LG * THREADS == RS * UG && XT % 64 == 0 && XT <= THREADS && (RS == 32 || RS == 64), "tile");
  static_assert(XT * 64 <= RING, "sums partials reuse the ring");
  // the element pass's per-channel constants (xform scale | shift, the BatchNorm's affine pair, mean): registers, or
  // at K = 512 -- where w's fragments and the dW accumulators take 128 -- a 5 x 64 fp32 table behind the staging tile
  constexpr bool PLDS = K > 256;
  __shared__ __attribute__((aligned(1024))) char smem[RING + IMG_X + (PLDS ? 5 * CT * 4 : 0) + (TLDS ? 3 * K * 4 : 0)];
  static_assert(sizeof(smem) <= 160 * 1024, "LDS");
  char* stg = smem + RING;
  float* ptab = reinterpret_cast<float*>(stg + IMG_X);
  float* btab = ptab + (PLDS ? 5 * CT : 0);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bid = blockIdx.x;
  int pair = bid, chalf = 0;
  if constexpr (HALVES == 2) {  // the two halves of a pair: one XCD, adjacent in dispatch order
    const int slot = bid >> 3;
    chalf = slot & 1;
    pair = (slot >> 1) * 8 + (bid & 7);
  }
  const int c0 = chalf * CT;
  const int n = pair < a.ntiles ? (a.ntiles - pair + a.npairs - 1) / a.npairs : 0;
  if (n == 0) return;
  const long M = a.M;
  const int C = a.C;

  // ---- w fragments of this wave's 16 channels: A operand of dz^T = w^T gy^T (row = channel, k = 8 (l >> 4) + j)
  const int ct = wid & 3, rh = wid >> 2;
  int4_t wf[NKS];
  {
    const uint16_t* wp = a.w + (long)(8 * (lane >> 4)) * C + c0 + ct * 16 + (lane & 15);
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      bf16x8_t v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (short)wp[(long)(ks * 32 + j) * C];
      wf[ks] = __builtin_bit_cast(int4_t, v);
    }
  }
  // ---- the element pass's channels: unit (tid & 7) of row tid >> 3 holds logical unit u of the 64
  const int erow = tid >> 3;
  const int eu = (tid & 7) ^ swz128(erow);
  const int ecol = c0 + eu * 8;
  float xsc[8], xsh[8], gsc[8], gsh[8], mu[8], ps[8], pq[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = a.mean[ecol + j];
    if constexpr (!FINAL) {
      xsc[j] = a.xform[ecol + j];
      xsh[j] = a.xform[C + ecol + j];
      bn_affine_regs(a.gamma[ecol + j], a.beta[ecol + j], mu[j], a.invstd[ecol + j], gsc[j], gsh[j]);
    } else {
      xsc[j] = xsh[j] = gsc[j] = gsh[j] = 0.f;  // (unused: x is the dW operand as stored, the ReLU decision a bit)
    }
    ps[j] = pq[j] = 0.f;
  }
  if constexpr (PLDS) {
    if (tid < 8) {  // row 0: swz128(0) = 0, unit tid
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ptab[0 * CT + tid * 8 + j] = xsc[j];
        ptab[1 * CT + tid * 8 + j] = xsh[j];
        ptab[2 * CT + tid * 8 + j] = gsc[j];
        ptab[3 * CT + tid * 8 + j] = gsh[j];
        ptab[4 * CT + tid * 8 + j] = mu[j];
      }
    }
  }
  // ---- ONLOAD: the channel unit of this thread's LG units of the gy image, and its constants
  const int tup = tid % UG, trow = tid / UG;
  float tsc[8], tB[8], tD[8];
  if constexpr (TREG) {
    const float* t = a.params + (tup ^ swz_g(trow)) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      tsc[j] = t[j];
      tB[j] = t[K + j];
      tD[j] = t[2 * K + j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(tsc[j]), "+v"(tB[j]), "+v"(tD[j]));
  }
  if constexpr (TLDS) {
    static_assert(!TLDS || PLDS, "the table's stores are ordered by the PLDS barrier");
    for (int i = tid; i < 3 * K; i += THREADS) btab[i] = a.params[i];
  }
  // every ordinary load is consumed here, before the first LDS-DMA is issued
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) asm volatile("" : "+v"(wf[ks]));
  if constexpr (FINAL) {
#pragma unroll
    for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(mu[j]));
  } else if constexpr (!PLDS) {
#pragma unroll
    for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(xsc[j]), "+v"(xsh[j]), "+v"(gsc[j]), "+v"(gsh[j]), "+v"(mu[j]));
  } else {
    __syncthreads();  // (the table's global loads are consumed by its LDS stores)
  }

  auto issue = [&](int slot, int i) {
    char* st = smem + slot * STAGE;
    const long m0 = (long)(pair + i * a.npairs) * RS;
    if constexpr (ONLOAD) {
      // rows past M read the tile's last valid row instead of the zero line -- a workgroup-uniform base and a 32-bit
      // offset per lane, which the registers this form has left need -- and the transform pass zeroes them
      const unsigned last = (unsigned)min((long)RS - 1, M - 1 - m0);
      const uint16_t* gb = a.gy + m0 * K;
      const uint16_t* xb = a.x3 + m0 * K;
#pragma unroll
      for (int j = 0; j < LG; ++j) {
        const unsigned row = j * (THREADS / UG) + trow;
        const unsigned off = min(row, last) * K + (tup ^ swz_g(row)) * 8;
        glds16(gb + off, st + j * (THREADS * 16) + wid * 1024);
        glds16(xb + off, st + IMG_G + j * (THREADS * 16) + wid * 1024);
      }
      if (wid < IMG_M / 1024) {  // the tile's mask rows are contiguous: lane = 16 B of row q * 16 / UG
        const unsigned q = (wid * 64 + lane) * 16;
        glds16(a.mask + m0 * UG + min(q / UG, last) * UG + q % UG, st + 2 * IMG_G + wid * 1024);
      }
      if (wid < XT / 64) {
        const unsigned eoff = min((unsigned)erow, last) * C + ecol;
        glds16(a.x + m0 * C + eoff, st + OFF_X + wid * 1024);
        if constexpr (FINAL) {
          glds16(a.addend + m0 * C + eoff, st + OFF_A + wid * 1024);
          glds16(a.xw + m0 * C + eoff, st + OFF_W + wid * 1024);
        }
      }
      if constexpr (FINAL) {  // lane = 4 B of row lane / 2
        if (wid == THREADS / 64 - 1)
          glds4(a.bits + m0 * 8 + min((unsigned)lane >> 1, last) * 8 + (lane & 1) * 4, st + OFF_B);
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < LG; ++j) {
      const int sl = j * THREADS + tid, row = sl / UG, up = sl % UG;
      const int u = up ^ swz_g(row);
      const long m = m0 + row;
      const void* src = m < M ? (const void*)(a.gy + m * K + u * 8) : (const void*)g_zero16;
      glds16(src, st + j * (THREADS * 16) + wid * 1024);
    }
    if (wid < XT / 64) {
      const long m = m0 + erow;
      const void* src = m < M ? (const void*)(a.x + m * C + ecol) : (const void*)g_zero16;
      glds16(src, st + OFF_X + wid * 1024);
      if constexpr (FINAL) {
        glds16(m < M ? (const void*)(a.addend + m * C + ecol) : (const void*)g_zero16, st + OFF_A + wid * 1024);
        glds16(m < M ? (const void*)(a.xw + m * C + ecol) : (const void*)g_zero16, st + OFF_W + wid * 1024);
      }
    }
    if constexpr (FINAL) {  // lane = 4 B of row lane / 2
      if (wid == THREADS / 64 - 1) {
        const long m = m0 + (lane >> 1);
        glds4(m < M ? (const void*)(a.bits + m * 8 + (lane & 1) * 4) : (const void*)g_zero16, st + OFF_B);
      }
    }
  };

  f32x4_t dwa[KTW][4];
#pragma unroll
  for (int i = 0; i < KTW; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) dwa[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int pre = min(n, NSLOT - 1);
  for (int s = 0; s < pre; ++s) issue(s, s);
  int slot = 0;
  for (int s = 0; s < n; ++s) {
    // stage s landed: of the younger stages in flight each wave counts the LPS loads every wave issues per stage (the
    // x and mask loads of the waves that have one, and the dz stores, only make the wait stricter). ONLOAD's two-slot
    // ring never has a younger stage in flight here -- stage s + 1 is issued below, after the barrier -- so its wait
    // is always vmcnt(0), whatever a stage's load count.
    const int younger = min(n - 1, s + NSLOT - 2) - s;
    if (younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPS) : "memory");
    else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPS) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();  // every wave's share of stage s is in LDS; stage s-1's reads are done
    if (s + NSLOT - 1 < n) issue(slot == 0 ? NSLOT - 1 : slot - 1, s + NSLOT - 1);  // into the slot of stage s-1
    char* G = smem + slot * STAGE;
    char* X = G + OFF_X;

    // ---- ONLOAD: the dy image becomes dx3 = bf16(fma(sc, mask ? dy : 0, fma(B, x3, D))) in place, unit by unit (the
    // expression and rounding of bn_bwd_apply_kernel); rows past M become the zero rows the rest relies on
    if constexpr (ONLOAD) {
      const int last = (int)min((long)RS - 1, M - 1 - (long)(pair + s * a.npairs) * RS);
#pragma unroll
      for (int j = 0; j < LG; ++j) {
        const int row = j * (THREADS / UG) + trow;
        const int u = tup ^ swz_g(row);
        char* gp = G + j * (THREADS * 16) + tid * 16;
        const bf16x8_t gv = *reinterpret_cast<const bf16x8_t*>(gp);
        const bf16x8_t xv = *reinterpret_cast<const bf16x8_t*>(gp + IMG_G);
        const uint32_t bits = *reinterpret_cast<const uint8_t*>(G + 2 * IMG_G + row * UG + u);
        float o[8];
#pragma unroll
        for (int h = 0; h < 8; h += 4) {  // (TLDS: 12 table values live at a time, not 24 -- w and dW hold 128)
          if constexpr (TLDS) {
            const float* t = btab + u * 8 + h;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              tsc[h + i] = t[i];
              tB[h + i] = t[K + i];
              tD[h + i] = t[2 * K + i];
            }
          }
#pragma unroll
          for (int i = h; i < h + 4; ++i) {
            const float g = (bits >> i) & 1u ? bf2f((uint16_t)gv[i]) : 0.f;
            o[i] = __builtin_fmaf(tsc[i], g, __builtin_fmaf(tB[i], bf2f((uint16_t)xv[i]), tD[i]));
            o[i] = row <= last ? o[i] : 0.f;
          }
          if constexpr (TLDS) asm volatile("" ::: "memory");  // (the next table reads stay behind this half's use)
        }
        *reinterpret_cast<bf16x8_t*>(gp) = pack_bf16x8(o);
      }
      lds_barrier();  // the dx3 tile is complete
    }

    // ---- dz tile: rows rh * RS/2 .., channels ct * 16 ..; lane holds row (l & 15), channels 4 (l >> 4) + r
    {
      f32x4_t d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
      const int row0 = rh * (RS / 2) + (lane & 15);
      const int kq = lane >> 4;
      if constexpr (RS == 64) {
        const int row1 = row0 + 16;
        const char* p0 = G + row0 * RB;
        const char* p1 = G + row1 * RB;
        const int s0 = swz_g(row0), s1 = swz_g(row1);
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          const bf16x8_t b0 = *reinterpret_cast<const bf16x8_t*>(p0 + (((ks * 4 + kq) ^ s0) << 4));
          const bf16x8_t b1 = *reinterpret_cast<const bf16x8_t*>(p1 + (((ks * 4 + kq) ^ s1) << 4));
          const mfma_bf16x8 wa = __builtin_bit_cast(mfma_bf16x8, wf[ks]);
          d0 = mfma16(wa, __builtin_bit_cast(mfma_bf16x8, b0), d0);
          d1 = mfma16(wa, __builtin_bit_cast(mfma_bf16x8, b1), d1);
        }
      } else {
        const char* p0 = G + row0 * RB;
        const int s0 = swz_g(row0);
#pragma unroll
        for (int ks = 0; ks < NKS; ks += 2) {
          const bf16x8_t b0 = *reinterpret_cast<const bf16x8_t*>(p0 + (((ks * 4 + kq) ^ s0) << 4));
          const bf16x8_t b1 = *reinterpret_cast<const bf16x8_t*>(p0 + (((ks * 4 + 4 + kq) ^ s0) << 4));
          d0 = mfma16(__builtin_bit_cast(mfma_bf16x8, wf[ks]), __builtin_bit_cast(mfma_bf16x8, b0), d0);
          d1 = mfma16(__builtin_bit_cast(mfma_bf16x8, wf[ks + 1]), __builtin_bit_cast(mfma_bf16x8, b1), d1);
        }
        d0 += d1;
      }
      const int unit = ct * 2 + (lane >> 5), half = (lane >> 4) & 1;
      auto put = [&](int row, const f32x4_t& d) {
        bf16x4_t o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (short)f2bf(d[r]);
        *reinterpret_cast<bf16x4_t*>(stg + row * 128 + ((unit ^ swz128(row)) << 4) + half * 8) = o;
      };
      put(row0, d0);
      if constexpr (RS == 64) put(row0 + 16, d1);
    }
    lds_barrier();  // the staged dz tile is complete

    // ---- element pass: store dz, add the sums, z over x in place
    if constexpr (FINAL) {
      // ---- element pass, final form: out = bf16(staged bf16 product + addend) -- the rounding of the tile kernel's
      // accumulating epilogue (gemm.hip), whose launch this one replaces -- stored over the addend, and the sums over
      // g = bit ? stored out : 0 against the winner's x (rows past M: no store, no sums -- their out is an addend the
      // clamped loads repeated); x stays as stored
      if (wid < XT / 64) {
        const bf16x8_t dzv = *reinterpret_cast<const bf16x8_t*>(stg + tid * 16);
        const bf16x8_t adv = *reinterpret_cast<const bf16x8_t*>(G + OFF_A + tid * 16);
        const bf16x8_t xv = *reinterpret_cast<const bf16x8_t*>(G + OFF_W + tid * 16);
        const long m = (long)(pair + s * a.npairs) * RS + erow;
        const uint32_t bits = m < M ? (uint32_t) * reinterpret_cast<const uint8_t*>(G + OFF_B + erow * 8 + eu) : 0u;
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = bf2f((uint16_t)dzv[j]) + bf2f((uint16_t)adv[j]);
        const bf16x8_t ov = pack_bf16x8(o);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float g = (bits >> j) & 1u ? bf2f((uint16_t)ov[j]) : 0.f;
          ps[j] += g;
          pq[j] = __builtin_fmaf(g, bf2f((uint16_t)xv[j]) - mu[j], pq[j]);
        }
        if (m < M) *reinterpret_cast<bf16x8_t*>(a.dz + m * C + ecol) = ov;
      }
    } else if (wid < XT / 64) {
      const bf16x8_t dzv = *reinterpret_cast<const bf16x8_t*>(stg + tid * 16);
      const bf16x8_t xv = *reinterpret_cast<const bf16x8_t*>(X + tid * 16);
      if constexpr (PLDS) {
        const float* t = ptab + (ecol - c0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          xsc[j] = t[j];
          xsh[j] = t[CT + j];
          gsc[j] = t[2 * CT + j];
          gsh[j] = t[3 * CT + j];
          mu[j] = t[4 * CT + j];
        }
      }
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xf = bf2f((uint16_t)xv[j]);
        o[j] = fmaxf(__builtin_fmaf(xf, xsc[j], xsh[j]), 0.f);
        const float g = relu_on(xf, gsc[j], gsh[j]) ? bf2f((uint16_t)dzv[j]) : 0.f;
        ps[j] += g;
        pq[j] = __builtin_fmaf(g, xf - mu[j], pq[j]);
      }
      *reinterpret_cast<bf16x8_t*>(X + tid * 16) = pack_bf16x8(o);
      const long m = (long)(pair + s * a.npairs) * RS + erow;
      if (m < M) *reinterpret_cast<bf16x8_t*>(a.dz + m * C + ecol) = dzv;
    }
    lds_barrier();  // the z tile is complete, the staging tile free

    // ---- dW: rows wid * KW .. of dW (gy columns) x 64 channels
#pragma unroll
    for (int kk = 0; kk < RS / 32; ++kk) {
      TrRaw ar[KTW], br[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) tr_load<128, swz128>(br[j], X, j * 16, kk, lane);
#pragma unroll
      for (int i = 0; i < KTW; ++i) tr_load<RB, swz_g>(ar[i], G, wid * KW + i * 16, kk, lane);
      K8S_LDS_TIE8("s_waitcnt lgkmcnt(0)", br[0].lo, br[0].hi, br[1].lo, br[1].hi, br[2].lo, br[2].hi, br[3].lo,
                   br[3].hi);
#pragma unroll
      for (int i = 0; i < KTW; i += 2)
        K8S_LDS_TIE4("s_waitcnt lgkmcnt(0)", ar[i].lo, ar[i].hi, ar[i + 1].lo, ar[i + 1].hi);
#pragma unroll
      for (int i = 0; i < KTW; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          dwa[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(join8(br[j].lo, br[j].hi), join8(ar[i].lo, ar[i].hi),
                                                              dwa[i][j], 0, 0, 0);
    }
    slot = slot + 1 == NSLOT ? 0 : slot + 1;
  }

  // ---- dW partials: lane holds dW[k = wid * KW + i * 16 + (lane & 15)][c0 + j * 16 + 4 (lane >> 4) + r]
  if constexpr (FINAL) {
    // this workgroup's slab, plain 16-B stores: the slabs are summed in workgroup order by splitk_reduce, so dW does
    // not depend on the order the workgroups finish in (the layer's weight gradient was a deterministic kernel's)
    float* slab = a.dwpart + (long)bid * K * CT;
#pragma unroll
    for (int i = 0; i < KTW; ++i) {
      const int k = wid * KW + i * 16 + (lane & 15);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        *reinterpret_cast<f32x4_t*>(slab + (long)k * CT + j * 16 + 4 * (lane >> 4)) = dwa[i][j];
    }
  } else
#pragma unroll
  for (int i = 0; i < KTW; ++i) {
    const int k = wid * KW + i * 16 + (lane & 15);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float* d = a.dw + (long)k * C + c0 + j * 16 + 4 * (lane >> 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) atomicAdd(d + r, dwa[i][j][r]);
    }
  }
  // ---- sums: the RS threads of a channel unit fold through LDS, one atomic per (channel, sum) per workgroup
  __syncthreads();
  float* part = reinterpret_cast<float*>(smem);
  if (tid < XT) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      part[tid * 16 + j] = ps[j];
      part[tid * 16 + 8 + j] = pq[j];
    }
  }
  __syncthreads();
  if (tid < 2 * CT) {
    const int col = tid & (CT - 1), which = tid / CT;
    const int u = col >> 3, r = col & 7;
    float v = 0.f;
#pragma unroll 4
    for (int row = 0; row < RS; ++row) v += part[(row * 8 + (u ^ swz128(row))) * 16 + which * 8 + r];
    atomicAdd(a.sums + (long)(bid % kConvStatReplicas) * 2 * C + (long)which * C + c0 + col, v);
  }
}

}  // namespace b1f

// The contract: (C, K) = (64, 256) or (128, 512), 1 <= M < 2^31.
bool bwd1x1_fused_ok(long M, int C, int K) {
  return M >= 1 && M < (1L << 31) && ((C == 64 && K == 256) || (C == 128 && K == 512));
}
// ... and of the final form (Bwd1x1Final): (C, K) = (64, 256) only
bool bwd1x1_final_ok(long M, int C, int K) { return bwd1x1_fused_ok(M, C, K) && C == 64; }
// fp32 elements of Bwd1x1Final::dw_partials: one [K][C] slab per workgroup that has a tile
long bwd1x1_final_workspace(long M, int C, int K) {
  return std::min<long>(std::max(1, planner_cus()), (M + 31) / 32) * K * C;
}

// bn3: null, or the residual BatchNorm's backward applied on load -- gy is then its incoming dy, and the kernel forms
// dx3 = fma(sc, mask ? dy : 0, fma(B, x3, D)) tile by tile instead of reading it (x3 [M][K] bf16, mask [M][K / 8]
// packed bits, params fp32 [sc | B | D], 3K or more).
// fin: null, or the final form -- x is the dW operand as stored (xform / gamma / beta / invstd null, mean unused), dz is
// fin->addend's storage, and the sums are the pool kind's over the stored sum.
void launch_bwd1x1_fused(const uint16_t* gy, const uint16_t* x, const uint16_t* w, const float* xform,
                         const float* gamma, const float* beta, const float* mean, const float* invstd, uint16_t* dz,
                         float* dw, float* sums, long M, int C, int K, bool accumulate, hipStream_t st,
                         const Bwd1x1Bn3* bn3, const Bwd1x1Final* fin) {
  using namespace b1f;
  if (!bwd1x1_fused_ok(M, C, K)) throw std::runtime_error("bwd1x1_fused: (C, K) = (64, 256) or (128, 512), M < 2^31");
  if (bn3 && !(bn3->x3 && bn3->mask && bn3->params)) throw std::runtime_error("bwd1x1_fused: x3, mask and params");
  if (fin) {
    if (!bwd1x1_final_ok(M, C, K)) throw std::runtime_error("bwd1x1_fused, final form: (C, K) = (64, 256)");
    if (!(fin->addend && fin->winner_x && fin->winner_bits && fin->winner_mean) || dz != fin->addend)
      throw std::runtime_error("bwd1x1_fused, final form: addend (the output), winner_x, winner_bits, winner_mean");
    if (xform || gamma || beta || mean || invstd)
      throw std::runtime_error("bwd1x1_fused, final form: no xform operands");
  }
  if (fin && !fin->dw_partials) throw std::runtime_error("bwd1x1_fused, final form: dw_partials");
  if (!accumulate && !fin) (void)hipMemsetAsync(dw, 0, (size_t)K * C * sizeof(float), st);
  Args a{gy, x, w, nullptr, nullptr, nullptr, xform, gamma, beta, mean, invstd, dz, dw, sums, (int)M, C, 0, 0,
         nullptr, nullptr, nullptr, nullptr};
  if (bn3) a.x3 = bn3->x3, a.mask = bn3->mask, a.params = bn3->params;
  const int cus = std::max(1, planner_cus());
  if (fin) {
    a.mean = fin->winner_mean, a.addend = fin->addend, a.xw = fin->winner_x, a.bits = fin->winner_bits;
    a.dwpart = fin->dw_partials;
    a.ntiles = (int)((M + 31) / 32);
    a.npairs = cus;
    if (bn3) hipLaunchKernelGGL((bwd1x1_fused_kernel<256, 32, 3, 1, true, true>), dim3(cus), dim3(THREADS), 0, st, a);
    else hipLaunchKernelGGL((bwd1x1_fused_kernel<256, 32, 4, 1, false, true>), dim3(cus), dim3(THREADS), 0, st, a);
    // workgroups 0 .. min(cus, ntiles) - 1 each wrote a slab: dw (+)= their sum, in that order
    splitk_reduce(fin->dw_partials, std::min(cus, a.ntiles), (long)K * C, dw, accumulate, st);
  } else if (C == 64) {
    a.ntiles = (int)((M + 63) / 64);
    a.npairs = cus;
    if (bn3) hipLaunchKernelGGL((bwd1x1_fused_kernel<256, 64, 2, 1, true>), dim3(cus), dim3(THREADS), 0, st, a);
    else hipLaunchKernelGGL((bwd1x1_fused_kernel<256, 64, 3, 1, false>), dim3(cus), dim3(THREADS), 0, st, a);
  } else {
    const int grid = std::max(16, cus / 16 * 16);  // pairs of workgroups, 8 pairs (one per XCD) at a time
    a.ntiles = (int)((M + 31) / 32);
    a.npairs = grid / 2;
    if (bn3) hipLaunchKernelGGL((bwd1x1_fused_kernel<512, 32, 2, 2, true>), dim3(grid), dim3(THREADS), 0, st, a);
    else hipLaunchKernelGGL((bwd1x1_fused_kernel<512, 32, 4, 2, false>), dim3(grid), dim3(THREADS), 0, st, a);
  }
}

}  // namespace k8s_amd
