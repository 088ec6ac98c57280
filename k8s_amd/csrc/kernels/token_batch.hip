// Token batch assembly: a whole BERT pretraining batch (mlm_batch_kernel) or a causal-LM batch (causal_batch_kernel;
// causal_doc_batch_kernel with the document bounds, positions and boundary-aware labels of document-masked attention)
// from the token array and a small host table, in one launch. Integer arithmetic only: ops/reference.py mlm_batch /
// causal_batch / causal_doc_batch are the same definitions in torch and match bit for bit.
//
// src    uint16 or int32 [T]   the split's tokens (or one staged batch of them)
// table  int64 [N][6]          per sample (a0, la, b0, lb, n, ord), drawn on the host (data/token_sampler.py)
//
// Sample row, position j, L = la + lb + 3:
//   tok[j]  = cls (0) | src[a0 + j - 1] (1 .. la) | sep (la + 1) | src[b0 + j - la - 2] (la + 2 .. la + lb + 1)
//             | sep (L - 1) | pad (L ..)
//   type[j] = 1 for la + 2 <= j <= L - 1, else 0
//   keys    : philox_rowkey(seed, 0, 3 * stream + {0, 1, 2}, ord) = ksel, kdec, krep; G = 0x9E3779B1
//   score[j]= mix32(ksel ^ j G); the n candidates (A and B positions) with the smallest (score, j) are selected;
//             a selected j's slot = selected positions below it: positions[slot] = j, labels[slot] = tok[j];
//             slots >= n: position 0, label -100
//   id[j]   = selected: u = mix32(kdec ^ j G) < 0.8 2^32 ? mask : u < 0.9 2^32 ? umulhi(mix32(krep ^ j G), vocab)
//             : tok[j]; unselected: tok[j]
//
// One wave per sample, four samples per 256-thread block. Lane l holds positions l, l + 64, ... (at most 8 at
// S <= 512), so a segment's token loads and the int64 stores are consecutive across the wave. The three Philox calls
// are wave-uniform. Scores go to the wave's LDS row; each lane then ranks its positions in one loop over the
// candidates of that row -- every lane reads the same address, a broadcast -- S^2 / 64 compares per lane. Slots
// come from one __ballot per 64-position chunk and __popcll of the lower lanes and the earlier chunks. Stores: the
// unused slots get their defaults, the selected lanes scatter theirs; plain vector stores, no atomics.
//
// UNPAD (mlm_batch_unpadded): the same samples written back to back into one stream of Tt rows. cu int64 [N + 1] holds
// the samples' first stream rows (cu[n + 1] - cu[n] = L_n). Sample n writes ids, types and pos = j at row cu[n] + j for
// j < L_n, with the span bounds lo = cu[n], hi = cu[n + 1] of ops.attention's span mask; labels are unchanged, the
// [N, P] positions become stream rows cu[n] + j (unused slots: cu[n]), and cls_rows[n] = cu[n]. Block 0 also writes the
// tail [cu[N], Tt), fewer than 128 rows: pad, type 0, pos 0, lo = cu[N], hi = Tt -- one pad span no real query sees.
// Selection, replacement and slots are the code below, shared: sample n gets the same masks padded and unpadded.
//
// Every source index is clamped into [0, T) and every length into the row here as well as validated on the host: no
// table content reads outside src or writes outside the outputs (UNPAD: every cu entry is clamped into [0, Tt] and
// every stream row is tested against Tt).
#include <stdexcept>

#include "common.h"
#include "launchers.h"
#include "rng.h"

namespace k8s_amd {

constexpr int kTokMaxS = 512, kTokChunks = kTokMaxS / 64;
constexpr uint32_t kTokG = 0x9E3779B1u;
constexpr uint32_t kTokMask80 = 3435973837u;  // floor(0.8 * 2^32 + 0.5)
constexpr uint32_t kTokMask90 = 3865470566u;  // floor(0.9 * 2^32 + 0.5)

__device__ __forceinline__ long tok_clamp(long v, long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <typename T>
__device__ __forceinline__ int tok_load(const T* __restrict__ src, long i, long Tn) {
  return (int)src[tok_clamp(i, Tn - 1)];  // uint16_t widens unsigned
}

// the stream outputs of the UNPAD form (unused, all null, by the padded one)
struct TokUnpad {
  const long* cu;  // [N + 1] on the device
  long Tt;         // stream rows
  long *pos, *cls_rows;
  int *lo, *hi;
};

template <typename T, bool UNPAD>
__global__ void __launch_bounds__(256) mlm_batch_kernel(const T* __restrict__ src, long Tn,
                                                        const long* __restrict__ table, int N, int S, int P,
                                                        uint32_t vocab, TokSpecial sp, uint64_t seed, int stream,
                                                        long* __restrict__ ids, long* __restrict__ types,
                                                        long* __restrict__ labels, long* __restrict__ positions,
                                                        TokUnpad up) {
  __shared__ uint32_t score_lds[4][kTokMaxS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int sample = blockIdx.x * 4 + wave;
  const bool live = sample < N;  // wave-uniform; a dead wave still meets the barrier
  const long* row = table + (long)(live ? sample : 0) * 6;
  long base = 0, end = 0;  // (UNPAD) the sample's stream rows [base, end)
  if constexpr (UNPAD) {
    base = tok_clamp(up.cu[live ? sample : 0], up.Tt);
    end = tok_clamp(up.cu[(live ? sample : 0) + 1], up.Tt);
    if (blockIdx.x == 0 && threadIdx.x < 128) {  // the tail
      const long t0 = tok_clamp(up.cu[N], up.Tt), e = t0 + threadIdx.x;
      if (e < up.Tt) {
        ids[e] = sp.pad;
        types[e] = 0;
        up.pos[e] = 0;
        up.lo[e] = (int)t0;
        up.hi[e] = (int)up.Tt;
      }
    }
  }
  const long a0 = row[0], b0 = row[2];
  const int la = (int)tok_clamp(row[1], S), lb = (int)tok_clamp(row[3], S - la);
  const int n = (int)tok_clamp(row[4], P);
  const uint64_t ord = (uint64_t)row[5];
  const int L = la + lb + 3;
  const uint32_t ksel = philox_rowkey(seed, 0, 3u * stream + 0u, ord);
  const uint32_t kdec = philox_rowkey(seed, 0, 3u * stream + 1u, ord);
  const uint32_t krep = philox_rowkey(seed, 0, 3u * stream + 2u, ord);
  uint32_t* score = score_lds[wave];

  int tok[kTokChunks];
  uint32_t sc[kTokChunks];
  bool cand[kTokChunks];
#pragma unroll
  for (int c = 0; c < kTokChunks; ++c) {
    const int j = c * 64 + lane;
    const bool inA = j >= 1 && j <= la, inB = j >= la + 2 && j <= la + lb + 1;
    int t = sp.pad;
    if (j < S) {  // wave-uniform per chunk except in the last one
      if (inA) t = tok_load(src, a0 + j - 1, Tn);
      if (inB) t = tok_load(src, b0 + j - la - 2, Tn);
    }
    if (j == 0) t = sp.cls;
    if (j == la + 1 || j == L - 1) t = sp.sep;
    tok[c] = t;
    cand[c] = (inA || inB) && j < S;
    sc[c] = drop_mix32(ksel ^ ((uint32_t)j * kTokG));
    if (j < S) score[j] = sc[c];
  }
  __syncthreads();

  // rank[c] = candidates k with (score[k], k) < (score[j], j): two runs of k, the A and the B positions
  int rank[kTokChunks];
#pragma unroll
  for (int c = 0; c < kTokChunks; ++c) rank[c] = 0;
  const int endA = min(la, S - 1), endB = min(la + lb + 1, S - 1);
  for (int k = 1; k <= endB; ++k) {
    if (k == endA + 1) {  // skip [SEP] between the runs (and everything past a clamped A)
      k = la + 1;
      continue;
    }
    const uint32_t s = score[k];
#pragma unroll
    for (int c = 0; c < kTokChunks; ++c) {
      const int j = c * 64 + lane;
      rank[c] += (s < sc[c] || (s == sc[c] && k < j)) ? 1 : 0;
    }
  }

  int nsel = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  long* lab = labels + (long)sample * P;
  long* pos = positions + (long)sample * P;
#pragma unroll
  for (int c = 0; c < kTokChunks; ++c) {
    const int j = c * 64 + lane;
    const bool sel = cand[c] && rank[c] < n;
    const unsigned long long bal = __ballot(sel);
    const int slot = nsel + __popcll(bal & below);
    nsel += __popcll(bal);
    int id = tok[c];
    if (sel) {
      const uint32_t jg = (uint32_t)j * kTokG;
      const uint32_t u = drop_mix32(kdec ^ jg);
      if (u < kTokMask80)
        id = sp.mask;
      else if (u < kTokMask90)
        id = (int)__umulhi(drop_mix32(krep ^ jg), vocab);
      if (live && slot < P) {
        lab[slot] = tok[c];
        pos[slot] = UNPAD ? base + j : j;
      }
    }
    const int type = (j >= la + 2 && j <= L - 1) ? 1 : 0;
    if constexpr (UNPAD) {
      const long e = base + j;
      if (live && j < S && j < L && e < up.Tt) {
        ids[e] = id;
        types[e] = type;
        up.pos[e] = j;
        up.lo[e] = (int)base;
        up.hi[e] = (int)end;
      }
    } else if (live && j < S) {
      ids[(long)sample * S + j] = id;
      types[(long)sample * S + j] = type;
    }
  }
  if (live) {
    for (int p = nsel + lane; p < P; p += 64) {  // the slots no selected position took
      lab[p] = -100;
      pos[p] = UNPAD ? base : 0;
    }
    if (UNPAD && lane == 0) up.cls_rows[sample] = base;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) causal_batch_kernel(const T* __restrict__ src, long Tn,
                                                           const long* __restrict__ starts, int S, int total,
                                                           long* __restrict__ ids, long* __restrict__ labels) {
  const int e = blockIdx.x * 256 + threadIdx.x;  // output element (n, j)
  if (e >= total) return;
  const long at = starts[e / S] + e % S;
  ids[e] = tok_load(src, at, Tn);
  labels[e] = tok_load(src, at + 1, Tn);
}

// causal_batch with document boundaries: element (n, j) sits at p = abs_starts[n] + j of the split; d is the largest
// index with doc_tok[d] <= p, clamped into [0, Dn - 1] (a binary search over the ascending offsets, at most 40 steps,
// every probe inside the table), and
//   lo = max(doc_tok[d] - abs, 0), hi = min(doc_tok[d + 1] - abs, S), pos = j - lo,
//   label = src[start + j + 1] if p + 1 < doc_tok[d + 1] else -100.
// The three int32 results are clamped into [0, S] / [-S, S] on their way out, which changes nothing for a window
// inside the split.
template <typename T>
__global__ void __launch_bounds__(256) causal_doc_batch_kernel(const T* __restrict__ src, long Tn,
                                                               const long* __restrict__ starts,
                                                               const long* __restrict__ abs_starts,
                                                               const long* __restrict__ doc_tok, int Dn, int S,
                                                               int total, long* __restrict__ ids,
                                                               long* __restrict__ labels, int* __restrict__ lo,
                                                               int* __restrict__ hi, int* __restrict__ pos) {
  const int e = blockIdx.x * 256 + threadIdx.x;  // output element (n, j)
  if (e >= total) return;
  const int n = e / S, j = e - n * S;
  const long at = starts[n] + j, ab = abs_starts[n], p = ab + j;
  int d = 0, top = Dn - 1;  // doc_tok[d] <= p < doc_tok[top + 1], or an end of the range
  for (int it = 0; it < 40 && d < top; ++it) {
    const int mid = (d + top + 1) >> 1;
    if (doc_tok[mid] <= p) d = mid;
    else top = mid - 1;
  }
  const long first = doc_tok[d], end = doc_tok[d + 1];
  const long l = tok_clamp(first - ab, S), h = tok_clamp(end - ab, S);
  ids[e] = tok_load(src, at, Tn);
  labels[e] = p + 1 < end ? tok_load(src, at + 1, Tn) : -100;
  lo[e] = (int)l;
  hi[e] = (int)h;
  pos[e] = (int)(j - l);
}

void launch_mlm_batch(const void* src, bool u16, long Tn, const long* table, int N, int S, int P, uint32_t vocab,
                      const TokSpecial& sp, uint64_t seed, int stream, long* ids, long* types, long* labels,
                      long* positions, hipStream_t st) {
  if (N < 1 || Tn < 1 || S < 1 || S > kTokMaxS || P < 1 || P > S || vocab < 2 || stream < 0)
    throw std::runtime_error("mlm_batch: bad shape");
  const dim3 grid(cdiv(N, 4)), block(256);
  const TokUnpad none{nullptr, 0, nullptr, nullptr, nullptr, nullptr};
  if (u16)
    hipLaunchKernelGGL((mlm_batch_kernel<uint16_t, false>), grid, block, 0, st, (const uint16_t*)src, Tn, table, N, S, P,
                       vocab, sp, seed, stream, ids, types, labels, positions, none);
  else
    hipLaunchKernelGGL((mlm_batch_kernel<int, false>), grid, block, 0, st, (const int*)src, Tn, table, N, S, P, vocab,
                       sp, seed, stream, ids, types, labels, positions, none);
}

void launch_mlm_batch_unpadded(const void* src, bool u16, long Tn, const long* table, const long* cu, long Tt, int N,
                               int S, int P, uint32_t vocab, const TokSpecial& sp, uint64_t seed, int stream, long* ids,
                               long* types, long* pos, long* labels, long* rows, long* cls_rows, int* lo, int* hi,
                               hipStream_t st) {
  if (N < 1 || Tn < 1 || S < 1 || S > kTokMaxS || P < 1 || P > S || vocab < 2 || stream < 0 || Tt < 1 ||
      Tt >= (1L << 31) || Tt % 128)
    throw std::runtime_error("mlm_batch_unpadded: bad shape");
  const dim3 grid(cdiv(N, 4)), block(256);
  const TokUnpad up{cu, Tt, pos, cls_rows, lo, hi};
  if (u16)
    hipLaunchKernelGGL((mlm_batch_kernel<uint16_t, true>), grid, block, 0, st, (const uint16_t*)src, Tn, table, N, S, P,
                       vocab, sp, seed, stream, ids, types, labels, rows, up);
  else
    hipLaunchKernelGGL((mlm_batch_kernel<int, true>), grid, block, 0, st, (const int*)src, Tn, table, N, S, P, vocab, sp,
                       seed, stream, ids, types, labels, rows, up);
}

void launch_causal_batch(const void* src, bool u16, long Tn, const long* starts, int N, int S, long* ids, long* labels,
                         hipStream_t st) {
  const long total = (long)N * S;
  if (N < 1 || Tn < 1 || S < 1 || total >= (1L << 31)) throw std::runtime_error("causal_batch: bad shape");
  const dim3 grid(cdiv(total, 256)), block(256);
  if (u16)
    hipLaunchKernelGGL(causal_batch_kernel<uint16_t>, grid, block, 0, st, (const uint16_t*)src, Tn, starts, S,
                       (int)total, ids, labels);
  else
    hipLaunchKernelGGL(causal_batch_kernel<int>, grid, block, 0, st, (const int*)src, Tn, starts, S, (int)total, ids,
                       labels);
}

void launch_causal_doc_batch(const void* src, bool u16, long Tn, const long* starts, const long* abs_starts,
                             const long* doc_tok, long Dn, int N, int S, long* ids, long* labels, int* lo, int* hi,
                             int* pos, hipStream_t st) {
  const long total = (long)N * S;
  if (N < 1 || Tn < 1 || S < 1 || Dn < 1 || Dn >= (1L << 31) - 1 || total >= (1L << 31))
    throw std::runtime_error("causal_doc_batch: bad shape");
  const dim3 grid(cdiv(total, 256)), block(256);
  if (u16)
    hipLaunchKernelGGL(causal_doc_batch_kernel<uint16_t>, grid, block, 0, st, (const uint16_t*)src, Tn, starts,
                       abs_starts, doc_tok, (int)Dn, S, (int)total, ids, labels, lo, hi, pos);
  else
    hipLaunchKernelGGL(causal_doc_batch_kernel<int>, grid, block, 0, st, (const int*)src, Tn, starts, abs_starts,
                       doc_tok, (int)Dn, S, (int)total, ids, labels, lo, hi, pos);
}

}  // namespace k8s_amd
