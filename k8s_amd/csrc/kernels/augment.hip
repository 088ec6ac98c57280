// Dataset batch assembly: gather + crop / resize + flip + normalise + bf16 + stem layout in one pass.
//
// src   uint8 [M][Hs][Ws][3]   the split (or one staged batch of it)
// table int32 [N][6]           per output sample (src index, y0, x0, h, w, flip), drawn on the host
// a, b  fp32 [3]               a_c = 1 / std_c, b_c = -mean_c / std_c
//
// Output element (n, i, j, c), jj = flip ? S-1-j : j:
//   h == S && w == S (copy row):  bf16(fmaf(src[idx][y0+i][x0+jj][c], a_c, b_c)), exactly 0 outside the source
//   otherwise (resized row):      the box [y0, y0+h) x [x0, x0+w) resized bilinearly to S x S (half-pixel centres,
//                                 indices clamped to the box, fp32 on the uint8 values: what F.interpolate(mode=
//                                 "bilinear", align_corners=False, antialias=False) computes), column jj, then the same
//                                 fmaf and one bf16 rounding
// Layouts: "nhwc8" [N][S][S][8] (channels 3..7 zero), one thread per 16-B pixel; "s2d" [N][S/2+3][S/2+3][16], the
// space-to-depth image stem_s2d_input_kernel makes of the nhwc8 image at pad 3, one thread per 32-B s2d pixel as
// there. Plain byte loads, 16-B vector stores.
//
// Read pattern: a wave covers 64 consecutive output columns of one row, so its byte loads fall into one run of
// 3 * 64 (nhwc8) or 6 * 64 (s2d: two adjacent source pixels per lane and row) consecutive source bytes, two or
// three 128-B lines per load instruction whatever the 3-byte pixel's alignment; a flipped row reads the same run
// in descending lane order, which costs no extra line. The nine to twelve byte loads of a lane hit lines its
// neighbours' loads brought in, so the source is fetched from L2 once. A resized row reads four taps per output
// pixel from at most two source rows: runs of w / S * 64 pixels, again contiguous.
//
// Every source coordinate is clamped here as well as validated on the host: no table content reads outside src.
#include <stdexcept>

#include "common.h"
#include "launchers.h"

namespace k8s_amd {

struct AugRow {
  const uint8_t* img;  // the sample's source image
  int y0, x0, h, w;
  bool flip, resize;
  float sy, sx;  // h / S, w / S
};

__device__ __forceinline__ int aug_clamp(int v, int hi) { return min(max(v, 0), hi); }

__device__ __forceinline__ AugRow aug_row(const uint8_t* __restrict__ src, const int* __restrict__ table, int n, int M,
                                          int Hs, int Ws, int S) {
  const int* t = table + (long)n * 6;
  AugRow r;
  r.img = src + (long)aug_clamp(t[0], M - 1) * Hs * Ws * 3;
  r.y0 = t[1];
  r.x0 = t[2];
  r.h = t[3];
  r.w = t[4];
  r.flip = t[5] != 0;
  r.resize = r.h != S || r.w != S;
  r.sy = (float)r.h / (float)S;
  r.sx = (float)r.w / (float)S;
  return r;
}

// normalised output pixel (i, j) of the S x S image of row r; 0 <= i, j < S
__device__ __forceinline__ void aug_pixel(const AugRow& r, int Hs, int Ws, int S, int i, int j, const AugNorm& nm,
                                          float (&o)[3]) {
  const int jj = r.flip ? S - 1 - j : j;
  if (!r.resize) {
    const int y = r.y0 + i, x = r.x0 + jj;
    const bool in = (unsigned)y < (unsigned)Hs && (unsigned)x < (unsigned)Ws;
    const uint8_t* p = r.img + ((long)aug_clamp(y, Hs - 1) * Ws + aug_clamp(x, Ws - 1)) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = in ? __builtin_fmaf((float)p[c], nm.a[c], nm.b[c]) : 0.f;
    return;
  }
  const float fy = fmaxf(((float)i + 0.5f) * r.sy - 0.5f, 0.f), fx = fmaxf(((float)jj + 0.5f) * r.sx - 0.5f, 0.f);
  const int iy0 = min((int)fy, r.h - 1), ix0 = min((int)fx, r.w - 1);
  const int iy1 = min(iy0 + 1, r.h - 1), ix1 = min(ix0 + 1, r.w - 1);
  const float ly = fy - (float)iy0, lx = fx - (float)ix0;
  const long ra = (long)aug_clamp(r.y0 + iy0, Hs - 1) * Ws, rb = (long)aug_clamp(r.y0 + iy1, Hs - 1) * Ws;
  const int xa = aug_clamp(r.x0 + ix0, Ws - 1), xb = aug_clamp(r.x0 + ix1, Ws - 1);
  const uint8_t* p00 = r.img + (ra + xa) * 3;
  const uint8_t* p01 = r.img + (ra + xb) * 3;
  const uint8_t* p10 = r.img + (rb + xa) * 3;
  const uint8_t* p11 = r.img + (rb + xb) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = (1.f - lx) * (float)p00[c] + lx * (float)p01[c];
    const float bot = (1.f - lx) * (float)p10[c] + lx * (float)p11[c];
    o[c] = __builtin_fmaf((1.f - ly) * top + ly * bot, nm.a[c], nm.b[c]);
  }
}

__global__ void __launch_bounds__(256) augment_nhwc8_kernel(const uint8_t* __restrict__ src,
                                                            const int* __restrict__ table, int M, int Hs, int Ws,
                                                            int S, AugNorm nm, uint16_t* __restrict__ out, int total) {
  const int e = blockIdx.x * 256 + threadIdx.x;  // output pixel (n, i, j)
  if (e >= total) return;
  const int j = e % S, t = e / S;
  const int i = t % S, n = t / S;
  const AugRow r = aug_row(src, table, n, M, Hs, Ws, S);
  float v[3];
  aug_pixel(r, Hs, Ws, S, i, j, nm, v);
  const float o[8] = {v[0], v[1], v[2], 0.f, 0.f, 0.f, 0.f, 0.f};
  *reinterpret_cast<bf16x8_t*>(out + (long)e * 8) = pack_bf16x8(o);
}

__global__ void __launch_bounds__(256) augment_s2d_kernel(const uint8_t* __restrict__ src,
                                                          const int* __restrict__ table, int M, int Hs, int Ws, int S,
                                                          AugNorm nm, uint16_t* __restrict__ out, int Ho,
                                                          int total) {
  const int e = blockIdx.x * 256 + threadIdx.x;  // s2d pixel (n, i, j) of [N][Ho][Ho][16], Ho = S / 2 + 3
  if (e >= total) return;
  const int j = e % Ho, t = e / Ho;
  const int i = t % Ho, n = t / Ho;
  const AugRow r = aug_row(src, table, n, M, Hs, Ws, S);
  bf16x8_t* dst = reinterpret_cast<bf16x8_t*>(out + (long)e * 16);
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    float o[8];
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int h = 2 * i + dy - 3, w = 2 * j + dx - 3;  // the stem's padding of 3
      const bool in = (unsigned)h < (unsigned)S && (unsigned)w < (unsigned)S;
      float v[3];
      aug_pixel(r, Hs, Ws, S, aug_clamp(h, S - 1), aug_clamp(w, S - 1), nm, v);
#pragma unroll
      for (int c = 0; c < 3; ++c) o[dx * 4 + c] = in ? v[c] : 0.f;
      o[dx * 4 + 3] = 0.f;
    }
    dst[dy] = pack_bf16x8(o);
  }
}

void launch_augment(const uint8_t* src, const int* table, int N, int M, int Hs, int Ws, int S, const AugNorm& nm,
                    bool s2d, uint16_t* out, hipStream_t st) {
  if (N < 1 || M < 1 || Hs < 1 || Ws < 1 || S < 1 || (s2d && S % 2)) throw std::runtime_error("augment: bad shape");
  const int Ho = S / 2 + 3;
  const long total = s2d ? (long)N * Ho * Ho : (long)N * S * S;
  if (total >= (1L << 31)) throw std::runtime_error("augment: too many output pixels");
  if (s2d)
    hipLaunchKernelGGL(augment_s2d_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, src, table, M, Hs, Ws, S, nm, out,
                       Ho, (int)total);
  else
    hipLaunchKernelGGL(augment_nhwc8_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, src, table, M, Hs, Ws, S, nm,
                       out, (int)total);
}

}  // namespace k8s_amd
