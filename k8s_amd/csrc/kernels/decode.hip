// Token-by-token generation (K16): the three kernels of a Llama decode step that the training kernels do not cover.
//
// A decode step multiplies every weight by an activation of 1 to 16 rows, so it is bound by the weight stream (and, in
// attention, by the K / V cache stream), never by arithmetic. All three kernels are plain streaming kernels: 16-byte
// loads straight into registers, no atomics, no scratch, and a work partition that is a function of the shapes alone
// (never of the grid or the device), so every result is bitwise repeatable.
//
//  * skinny_kernel (linear_skinny): y[M, N] = x[M, K] . w[N, K]^T for 1 <= M <= 16, K % 64 == 0, N % 16 == 0.
//    One wave owns 16 weight rows (a "wave tile"), a block of 4 waves 64 rows and one K chunk. The products go through
//    v_mfma_f32_16x16x32_bf16 with the 16 weight rows as the A operand and x (zero rows above M) as the 16-column B
//    operand. Why MFMA and not v_dot2c_f32_bf16: the kernel is bandwidth-bound either way, but a dot2c form needs one
//    accumulator per (row of x, weight row) pair -- up to 16 per lane and as many VALU instructions per 4 weight bytes
//    -- and a cross-lane sum at the end, where one MFMA retires 16 rows x 32 k against all 16 columns at once and its
//    result layout is already the output layout. A column of an MFMA depends on no other column, so row m's bits depend
//    neither on M nor on the other rows.
//    The k order inside an MFMA is free as long as both operands agree (mfma.h), so a lane takes k = 16 * (lane >> 4)
//    + 0..15 of each 64-wide step, two adjacent 16-byte loads in ONE weight row: the four lane groups of a weight row
//    cover a whole 128-byte line per step. Weights are read once and bypass the cache hierarchy's retention
//    (non-temporal loads). x is staged through LDS in fragment order (one ds_read_b128 per operand, lane-linear) and is
//    shared by the block's four waves.
//    When N / 64 blocks cannot fill the chip (the O projection of Llama-3-8B has 256 wave tiles) K is split into
//    chunks of KC = skinny_plan(N, K).kc, a function of (N, K) alone; every chunk writes an fp32 partial [M, N] and
//    skinny_fold_kernel adds them in chunk order and rounds once. Without a split the kernel rounds and stores itself.
//  * kv_append_kernel: token s of row b of the packed, rotated projection output goes to cache position start[b] + s,
//    clamped into [0, Smax - 1] (the host has checked the mirror of start; the clamp keeps a disagreeing device table
//    inside the cache). 16-byte loads and stores; serves prefill (S rows) and decode (S = 1).
//  * decode_attn_kernel / decode_merge_kernel: one block per (batch row, KV head, chunk of kDecodeChunk = 256 keys),
//    each of its 4 waves 64 keys. The scores of the group's up to 16 queries come from MFMAs with K rows as the A
//    operand (the skinny GEMM's fragment order), so every K byte is read once for the whole group; the softmax is per
//    wave; P . V runs on the vector ALU with V rows read by 16-byte loads (each lane 8 head-dim columns of one key, the
//    probabilities broadcast from LDS) -- V's MFMA operand would need the keys along a lane, a transposed read, and at
//    <= 16 queries the ALU keeps up with the stream. The block folds its waves and writes one fp32 partial (m, l, o)
//    per chunk; decode_merge_kernel combines a row's ceil(len / 256) chunks in chunk order. lens is read on the device
//    and clamped into [1, Smax]; a key index at or past len is clamped to len - 1 BEFORE it becomes an address, so
//    cache rows that were never written are never loaded, and its probability is an exact zero.
#include <stdexcept>

#include "launchers.h"
#include "mfma.h"

namespace k8s_amd {

namespace {

__device__ __forceinline__ mfma_bf16x8 ld16(const uint16_t* p) {
  return __builtin_bit_cast(mfma_bf16x8, *reinterpret_cast<const bf16x8_t*>(p));
}
__device__ __forceinline__ mfma_bf16x8 ld16_nt(const uint16_t* p) {
  return __builtin_bit_cast(mfma_bf16x8, __builtin_nontemporal_load(reinterpret_cast<const bf16x8_t*>(p)));
}

// --------------------------------------------------------------------------------------------------- skinny GEMM
constexpr int kSkinnySub = 512;  // k per staged piece of x: 8 steps of 64, 16 KB of LDS

template <bool PARTIAL>
__global__ void __launch_bounds__(256) skinny_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ w,
                                                     uint16_t* __restrict__ y, float* __restrict__ part, int M, int N,
                                                     int K, int KC) {
  __shared__ bf16x8_t xs[16 * 64];  // [step 0..7][half 0..1][lane]: the B fragments of one 512-k piece
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g4 = lane >> 4;
  const int tile = blockIdx.x * 4 + wave;
  const bool active = tile < N / 16;  // (a last block may hold fewer than four wave tiles; its other waves only stage)
  const int kbeg = blockIdx.y * KC, kend = min(K, kbeg + KC);
  const uint16_t* wrow = w + (long)(active ? tile * 16 + r16 : 0) * K + 16 * g4;
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  for (int ks = kbeg; ks < kend; ks += kSkinnySub) {
    const int nsteps = min(8, (kend - ks) >> 6);
    // this piece's weights first: 16 loads in flight per lane while x is staged
    mfma_bf16x8 wv[16];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (active && s < nsteps) {
        wv[2 * s] = ld16_nt(wrow + ks + 64 * s);
        wv[2 * s + 1] = ld16_nt(wrow + ks + 64 * s + 8);
      } else {
        wv[2 * s] = mfma_bf16x8{};
        wv[2 * s + 1] = mfma_bf16x8{};
      }
    }
    __syncthreads();  // the previous piece's fragment reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = threadIdx.x + 256 * i;
      const int m = q >> 6, c = q & 63, k = ks + 8 * c;  // 16-byte unit c of row m
      bf16x8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (m < M && k < kend) v = *reinterpret_cast<const bf16x8_t*>(x + (long)m * K + k);
      xs[((c >> 3) * 2 + (c & 1)) * 64 + ((c >> 1) & 3) * 16 + m] = v;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (s < nsteps) {
        acc = mfma16(wv[2 * s], __builtin_bit_cast(mfma_bf16x8, xs[(2 * s) * 64 + lane]), acc);
        acc = mfma16(wv[2 * s + 1], __builtin_bit_cast(mfma_bf16x8, xs[(2 * s + 1) * 64 + lane]), acc);
      }
    }
  }
  if (!active || r16 >= M) return;
  const long n = (long)tile * 16 + 4 * g4;  // this lane: row m = r16 of x, weight rows n .. n + 3
  if (PARTIAL) {
    *reinterpret_cast<f32x4_t*>(part + ((long)blockIdx.y * M + r16) * N + n) = acc;
  } else {
    bf16x4_t o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (short)f2bf(acc[r]);
    *reinterpret_cast<bf16x4_t*>(y + (long)r16 * N + n) = o;
  }
}

// y = bf16(part[0] + part[1] + ... in chunk order), 4 columns per thread
__global__ void __launch_bounds__(256) skinny_fold_kernel(const float* __restrict__ part, uint16_t* __restrict__ y,
                                                          long MN, int nsplit) {
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < MN; i += (long)gridDim.x * 1024) {
    f32x4_t a = *reinterpret_cast<const f32x4_t*>(part + i);
    for (int z = 1; z < nsplit; ++z) a += *reinterpret_cast<const f32x4_t*>(part + (long)z * MN + i);
    bf16x4_t o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (short)f2bf(a[r]);
    *reinterpret_cast<bf16x4_t*>(y + i) = o;
  }
}

// --------------------------------------------------------------------------------------------------- cache append
__global__ void __launch_bounds__(256) kv_append_kernel(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ ck,
                                                        uint16_t* __restrict__ cv, const int* __restrict__ start,
                                                        int B, int S, int Hq, int Hkv, int D, int Smax) {
  const int U = D / 8;  // 16-byte units of a head row
  const long total = (long)B * S * 2 * Hkv * U;
  const long W = (long)(Hq + 2 * Hkv) * D;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int u = (int)(i % U);
    long r = i / U;
    const int h = (int)(r % Hkv);
    r /= Hkv;
    const int which = (int)(r & 1);  // 0: key, 1: value
    r >>= 1;
    const int s = (int)(r % S), b = (int)(r / S);
    const int pos = min(max(start[b] + s, 0), Smax - 1);
    const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(qkv + ((long)b * S + s) * W +
                                                           (long)(Hq + which * Hkv + h) * D + 8 * u);
    uint16_t* dst = which ? cv : ck;
    *reinterpret_cast<bf16x8_t*>(dst + (((long)b * Hkv + h) * Smax + pos) * D + 8 * u) = v;
  }
}

// --------------------------------------------------------------------------------------------------- decode attention
// GP: the group's queries rounded up to 4 or 16 (the accumulator rows a lane carries in P . V)
template <int D, int GP>
__global__ void __launch_bounds__(256) decode_attn_kernel(const uint16_t* __restrict__ q,
                                                          const uint16_t* __restrict__ ck,
                                                          const uint16_t* __restrict__ cv,
                                                          const int* __restrict__ lens, float* __restrict__ ws_ml,
                                                          float* __restrict__ ws_o, long ldq, int Hq, int Hkv,
                                                          int Smax, float scale) {
  __shared__ float pl[4][64][GP];   // probabilities [wave][key][query]
  __shared__ float mo[4][GP][D];    // the waves' unnormalised outputs
  __shared__ float ml[4][GP][2];    // the waves' (max, sum)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g4 = lane >> 4;
  const int chunk = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int G = Hq / Hkv;
  const int len = min(max(lens[b], 1), Smax);
  if (chunk * kDecodeChunk >= len) return;  // (the whole block: no barrier has been reached)
  const int key0 = chunk * kDecodeChunk + wave * 64;  // (a wave past len computes on clamped rows, every key masked)
  const long head = ((long)b * Hkv + kvh) * Smax * D;

  // ---- scores: S[key, g] = K[key, :] . Q[g, :], four 16-key tiles
  mfma_bf16x8 qf[D / 64][2];
#pragma unroll
  for (int st = 0; st < D / 64; ++st)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      qf[st][h] = r16 < G ? ld16(q + b * ldq + (long)(kvh * G + r16) * D + 64 * st + 16 * g4 + 8 * h) : mfma_bf16x8{};
  f32x4_t sc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int key = min(key0 + 16 * t + r16, len - 1);  // the clamp comes before the address
    const uint16_t* kr = ck + head + (long)key * D + 16 * g4;
    f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < D / 64; ++st) {
      a = mfma16(ld16(kr + 64 * st), qf[st][0], a);
      a = mfma16(ld16(kr + 64 * st + 8), qf[st][1], a);
    }
    sc[t] = a;
  }
  // this lane: query r16, keys key0 + 16 t + 4 g4 + r
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool on = key0 + 16 * t + 4 * g4 + r < len;
      sc[t][r] = on ? sc[t][r] * scale : -INFINITY;
      mx = fmaxf(mx, sc[t][r]);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float mref = mx == -INFINITY ? 0.f : mx;
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = sc[t][r] == -INFINITY ? 0.f : __expf(sc[t][r] - mref);
      sum += p;
      if (r16 < GP) pl[wave][16 * t + 4 * g4 + r][r16] = p;
    }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  if (g4 == 0 && r16 < GP) {
    ml[wave][r16][0] = mx;
    ml[wave][r16][1] = sum;
  }
  __syncthreads();

  // ---- O[g, :] += P[g, key] V[key, :]: a lane holds 8 columns of one key per load
  constexpr int LPR = D / 8, KPI = 64 / LPR, NIT = 64 / KPI;  // lanes per V row, keys per load, loads
  const int u = lane % LPR, kk = lane / LPR;
  float o[GP][8];
#pragma unroll
  for (int g = 0; g < GP; ++g)
#pragma unroll
    for (int j = 0; j < 8; ++j) o[g][j] = 0.f;
#pragma unroll 1
  for (int i0 = 0; i0 < NIT; i0 += 4) {
    bf16x8_t vv[4];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      const int key = min(key0 + (i0 + ii) * KPI + kk, len - 1);
      vv[ii] = *reinterpret_cast<const bf16x8_t*>(cv + head + (long)key * D + 8 * u);
    }
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      const int kl = (i0 + ii) * KPI + kk;
      float vf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) vf[j] = bf2f((uint16_t)vv[ii][j]);
#pragma unroll
      for (int g4i = 0; g4i < GP / 4; ++g4i) {
        const f32x4_t p = *reinterpret_cast<const f32x4_t*>(&pl[wave][kl][4 * g4i]);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int j = 0; j < 8; ++j) o[4 * g4i + e][j] = __builtin_fmaf(p[e], vf[j], o[4 * g4i + e][j]);
      }
    }
  }
#pragma unroll
  for (int g = 0; g < GP; ++g)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = o[g][j];
#pragma unroll
      for (int off = LPR; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
      o[g][j] = v;
    }
  if (kk == 0) {
#pragma unroll
    for (int g = 0; g < GP; ++g)
#pragma unroll
      for (int j = 0; j < 8; ++j) mo[wave][g][8 * u + j] = o[g][j];
  }
  __syncthreads();

  // ---- the block's partial: its four waves in wave order
  const int NCH = gridDim.x;
  const long slot = ((long)b * Hkv + kvh) * NCH + chunk;
  for (int e = threadIdx.x; e < G * D; e += 256) {
    const int g = e / D, d = e % D;
    float M = ml[0][g][0];  // wave 0 of a live block always holds a key below len
#pragma unroll
    for (int w = 1; w < 4; ++w) M = fmaxf(M, ml[w][g][0]);
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float mw = ml[w][g][0];
      const float f = mw == -INFINITY ? 0.f : __expf(mw - M);
      L = __builtin_fmaf(ml[w][g][1], f, L);
      O = __builtin_fmaf(mo[w][g][d], f, O);
    }
    ws_o[(slot * G + g) * D + d] = O;
    if (d == 0) {
      ws_ml[(slot * G + g) * 2] = M;
      ws_ml[(slot * G + g) * 2 + 1] = L;
    }
  }
}

__global__ void __launch_bounds__(256) decode_merge_kernel(const float* __restrict__ ws_ml,
                                                           const float* __restrict__ ws_o,
                                                           const int* __restrict__ lens, uint16_t* __restrict__ out,
                                                           int Hq, int Hkv, int D, int Smax, int NCH) {
  const int kvh = blockIdx.x, b = blockIdx.y;
  const int G = Hq / Hkv;
  const int len = min(max(lens[b], 1), Smax);
  const int nc = min((len + kDecodeChunk - 1) / kDecodeChunk, NCH);  // the chunks that wrote a partial
  const long slot0 = ((long)b * Hkv + kvh) * NCH;
  for (int e = threadIdx.x; e < G * D; e += 256) {
    const int g = e / D, d = e % D;
    float M = -INFINITY;
    for (int c = 0; c < nc; ++c) M = fmaxf(M, ws_ml[((slot0 + c) * G + g) * 2]);
    float L = 0.f, O = 0.f;
    for (int c = 0; c < nc; ++c) {
      const float f = __expf(ws_ml[((slot0 + c) * G + g) * 2] - M);
      L = __builtin_fmaf(ws_ml[((slot0 + c) * G + g) * 2 + 1], f, L);
      O = __builtin_fmaf(ws_o[((slot0 + c) * G + g) * D + d], f, O);
    }
    out[((long)b * Hq + kvh * G + g) * D + d] = f2bf(O / L);
  }
}

}  // namespace

// --------------------------------------------------------------------------------------------------- host side
bool linear_skinny_ok(long M, long N, long K) {
  return M >= 1 && M <= 16 && K >= 64 && K % 64 == 0 && N >= 16 && N % 16 == 0 && N * K < (1L << 40) &&
         N < (1L << 27) && K < (1L << 24);
}

SkinnyPlan skinny_plan(long N, long K) {
  // K chunks until about kSkinnyBlocks blocks exist, a chunk never shorter than one staged piece: a function of the
  // shape alone
  constexpr long kSkinnyBlocks = 1024;
  const long nb = (N / 16 + 3) / 4, steps = K / 64;
  long want = (kSkinnyBlocks + nb - 1) / nb;
  const long most = K / kSkinnySub > 1 ? K / kSkinnySub : 1;
  if (want > most) want = most;
  if (want < 1) want = 1;
  const long per = (steps + want - 1) / want;
  SkinnyPlan p;
  p.kc = (int)(per * 64);
  p.nsplit = (int)((steps + per - 1) / per);
  return p;
}

void launch_linear_skinny(const uint16_t* x, const uint16_t* w, uint16_t* y, float* part, int M, int N, int K,
                          hipStream_t st) {
  if (!linear_skinny_ok(M, N, K)) throw std::runtime_error("linear_skinny: shape outside the kernel's contract");
  const SkinnyPlan p = skinny_plan(N, K);
  const dim3 grid((N / 16 + 3) / 4, p.nsplit);
  if (p.nsplit == 1) {
    hipLaunchKernelGGL(skinny_kernel<false>, grid, dim3(256), 0, st, x, w, y, nullptr, M, N, K, p.kc);
    return;
  }
  if (part == nullptr) throw std::runtime_error("linear_skinny: a split product needs its fp32 partials");
  hipLaunchKernelGGL(skinny_kernel<true>, grid, dim3(256), 0, st, x, w, y, part, M, N, K, p.kc);
  const long MN = (long)M * N;
  hipLaunchKernelGGL(skinny_fold_kernel, dim3(stream_grid(MN / 4, 256)), dim3(256), 0, st, part, y, MN, p.nsplit);
}

void launch_kv_append(const uint16_t* qkv, uint16_t* ck, uint16_t* cv, const int* start, int B, int S, int Hq, int Hkv,
                      int D, int Smax, hipStream_t st) {
  if (B < 1 || S < 1 || Hq < 1 || Hkv < 1 || D < 8 || D % 8 || Smax < 1)
    throw std::runtime_error("kv_append: bad shape");
  const long total = (long)B * S * 2 * Hkv * (D / 8);
  hipLaunchKernelGGL(kv_append_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, st, qkv, ck, cv, start, B, S, Hq,
                     Hkv, D, Smax);
}

void launch_decode_attention(const uint16_t* q, long ldq, const uint16_t* ck, const uint16_t* cv, const int* lens, float* ws_ml,
                             float* ws_o, uint16_t* out, int B, int Hq, int Hkv, int D, int Smax, int nchunks,
                             float scale, hipStream_t st) {
  if ((D != 64 && D != 128) || B < 1 || Hkv < 1 || Hq % Hkv || Hq / Hkv > 16 || Smax < 1 || nchunks < 1 ||
      (long)nchunks * kDecodeChunk >= (long)Smax + kDecodeChunk || B > 65535 || Hkv > 65535 || ldq < (long)Hq * D ||
      ldq % 8)
    throw std::runtime_error("decode_attention: shape outside the kernel's contract");
  const int G = Hq / Hkv;
  const dim3 grid(nchunks, Hkv, B);
#define K8S_DECODE_ATTN(DD, GG)                                                                                      \
  hipLaunchKernelGGL((decode_attn_kernel<DD, GG>), grid, dim3(256), 0, st, q, ck, cv, lens, ws_ml, ws_o, ldq, Hq, Hkv, \
                     Smax, scale)
  if (D == 64) {
    if (G <= 4) K8S_DECODE_ATTN(64, 4); else K8S_DECODE_ATTN(64, 16);
  } else {
    if (G <= 4) K8S_DECODE_ATTN(128, 4); else K8S_DECODE_ATTN(128, 16);
  }
#undef K8S_DECODE_ATTN
  hipLaunchKernelGGL(decode_merge_kernel, dim3(Hkv, B), dim3(256), 0, st, ws_ml, ws_o, lens, out, Hq, Hkv, D, Smax,
                     nchunks);
}

}  // namespace k8s_amd
