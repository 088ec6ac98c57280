// Host-side launcher declarations for every gfx950 kernel translation unit.
// The kernels themselves are compiled without any PyTorch headers (fast,
// parallel builds); only the files of csrc/binding see torch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rng.h"

namespace k8s_amd {

// planner.hip: the CU count every launch planner sizes its grid for (see common.h)
int planner_cus();
void set_planner_cus(int n);

// optim.hip
void launch_sgd(float* p, float* mom, const void* g, bool g_bf16, uint16_t* pbf, long n, const uint8_t* decay_mask, float lr,
                float mu, float wd, float scale, const float* scale_ptr, const float* hyper, bool nesterov,
                bool first_step, hipStream_t st);
void launch_adam(float* p, float* m1, float* m2, const void* g, bool g_bf16, uint16_t* pbf, long n, const uint8_t* decay_mask,
                 float lr, float b1, float b2, float eps, float wd, float scale, const float* scale_ptr,
                 const float* hyper, float bc1, float bc2, bool decoupled, hipStream_t st);
void launch_sumsq(const void* g, bool g_bf16, long n, float* out, hipStream_t st);
void launch_clip_factor(const float* stats, float max_norm, float* factor, hipStream_t st);
void launch_slice_sum(const uint16_t* in, long n, int world, float* out, uint16_t* out_bf, hipStream_t st);
void launch_cast_bf16(const float* in, uint16_t* out, long n, hipStream_t st);

// accum.hip: gradient accumulation over n elements (a multiple of 64) of two flat fp32 buffers.
// accumulate: acc = first ? g : acc + g. fold: g = g + acc, and out_bf = bf16(g) when given.
void launch_grad_accumulate(float* acc, const float* g, long n, bool first, hipStream_t st);
void launch_grad_fold(float* g, const float* acc, uint16_t* out_bf, long n, hipStream_t st);

// layerwise.hip: LARS / LAMB over a work-item table, items = long[n_items][4] {flat offset, state offset, length,
// segment}; flags = per-segment bits (1 decay, 2 low-precision copy); partial [n_items][2], sums [n_seg][2]
constexpr int kLayerItemMax = 16384;  // elements per work item, at most
void launch_layer_sums(const long* items, int n_items, const float* p, float* m1, float* m2, const void* g,
                       bool g_bf16, const uint8_t* flags, float* partial, bool lamb, float b1, float b2, float eps,
                       float wd, float scale, const float* scale_ptr, const float* hyper, float bc1, float bc2,
                       hipStream_t st);
void launch_layer_fold(const float* partial, const int* seg_start, int n_seg, float* sums, const float* scale_ptr,
                       hipStream_t st);
void launch_layer_ratio(const float* sums, const uint8_t* flags, int n_seg, float* ratio, bool lamb, float eta,
                        float wd, const float* scale_ptr, hipStream_t st);
void launch_layer_update(const long* items, int n_items, float* p, float* m1, const float* m2, const void* g,
                         bool g_bf16, uint16_t* pbf, const uint8_t* flags, const float* ratio, bool lamb, float lr,
                         float mu, float b1, float b2, float eps, float wd, float scale, const float* scale_ptr,
                         const float* hyper, float bc1, float bc2, bool first_step, hipStream_t st);

// batchnorm.hip
int bn_workspace_floats(long M, int C);
// params: fp32 workspace, [2][C] for the forward (scale, shift), [4][C] for the backward (sc, B, D, shift)
void launch_bn_fwd(const uint16_t* x, const uint16_t* res, const float* gamma, const float* beta, uint16_t* y,
                   float* save_mean, float* save_invstd, float* run_mean, float* run_var, float* work, float* params,
                   long M, int C, float eps, float momentum, bool training, bool relu, hipStream_t st,
                   uint8_t* mask = nullptr);
void launch_bn_fwd_from_sums(const uint16_t* x, const uint16_t* res, const float* gamma, const float* beta,
                             uint16_t* y, const float* sums, int nrep, float* save_mean, float* save_invstd,
                             float* run_mean, float* run_var, float* params, long M, int C, float eps, float momentum,
                             bool relu, hipStream_t st, uint8_t* mask = nullptr, uint16_t* ysub = nullptr,
                             int H = 1, int W = 1);
void launch_bn_fwd_from_sums_dual(const uint16_t* x, const float* gamma, const float* beta, const float* sums,
                                  int nrep, float* save_mean, float* save_invstd, float* run_mean, float* run_var,
                                  float* params, const uint16_t* xr, const float* gamma_r, const float* beta_r,
                                  const float* sums_r, int nrep_r, float* save_mean_r, float* save_invstd_r,
                                  float* run_mean_r, float* run_var_r, float* params_r, uint16_t* y, uint8_t* mask,
                                  long M, int C, float eps, float momentum, hipStream_t st);
// One BatchNorm of a backward. Two decisions describe every form: who did the reduction (this call: `work`; dy's
// producer: `sums`) and who runs the apply pass (this call: `dx`; x's producer as it loads dy: `dx` null).
struct BnBwdSide {
  const uint16_t* x = nullptr;
  const float *mean = nullptr, *invstd = nullptr, *gamma = nullptr, *beta = nullptr;
  float *dgamma = nullptr, *dbeta = nullptr;
  const float* sums = nullptr;  // the producer's reduction [nrep][2][C] (sum g, sum g (x - mean)), or null
  float* work = nullptr;        // the reduce sweep's partials (bn_workspace_floats); null when `sums` is given
  float* params = nullptr;      // fp32 [4][C] (sc | B | D | shift): written by the first half, read by the second
  uint16_t* dx = nullptr;       // where the apply pass writes; null: deferred to a consumer that applies on load
};
// The first half: dgamma, dbeta and the params table of `a` -- and of `b`, a second BatchNorm fed by the same masked
// dy (a ResNet downsample block; both sides with sums or both without; with sums `b` shares `a`'s sum g, slot 0).
// The ReLU of the forward: the packed `mask`, recomputed from x (`relu_x`, one side only), or none.
void launch_bn_bwd_params(const uint16_t* dy, const uint8_t* mask, bool relu_x, int nrep, const BnBwdSide& a,
                          const BnBwdSide* b, long M, int C, hipStream_t st);
// The second half: a.dx (and dres = the masked dy) from a.params; with `b` both dx in one pass over dy and the mask.
void launch_bn_bwd_apply(const uint16_t* dy, const uint8_t* mask, bool relu_x, const BnBwdSide& a, const BnBwdSide* b,
                         uint16_t* dres, long M, int C, hipStream_t st);
void launch_bn_finalize_sums(const float* gamma, const float* beta, const float* sums, int nrep, float* save_mean,
                             float* save_invstd, float* run_mean, float* run_var, float* params, long M, int C,
                             float eps, float momentum, hipStream_t st);
constexpr int kConvStatReplicas = 32;  // must match STAT_REPL in gemm.hip
// packed ReLU bits of a bf16 tensor (bit j of byte e = y[8e + j] > 0), nvec = numel / 8
void launch_relu_mask(const uint16_t* y, uint8_t* mask, long nvec, hipStream_t st);

// norm.hip
void launch_norm_fwd(bool rms, const uint16_t* x, const uint16_t* res, uint16_t* xsum, const float* gamma,
                     const float* beta, uint16_t* y, float* mean, float* rstd, long R, int D, float eps,
                     hipStream_t st, const DropArgs* drop = nullptr);
int norm_workspace_floats(long R, int D);
void launch_norm_bwd(bool rms, const uint16_t* dy, const uint16_t* x, const float* gamma, const float* mean,
                     const float* rstd, const uint16_t* dres, uint16_t* dx, float* dgamma, float* dbeta, float* work,
                     long R, int D, hipStream_t st, float* dsum = nullptr, const DropArgs* drop = nullptr,
                     uint16_t* da = nullptr);
// drop (LayerNorm with a residual only): the first summand passes through dropout before the add,
//   xsum = bf16(keep * scale * x + res); the backward also writes da = keep * scale * dx (the gradient of x; dx itself
//   is the residual's), and dsum becomes the column sums of da.

// dropout.hip: y = keep ? bf16(x * scale) : 0 over [R, D] bf16 (D % 8 == 0); the keep bits of rows row0 .. row0 + R - 1,
// columns 0 .. C - 1 as uint8 (rng.h)
void launch_dropout(const uint16_t* x, uint16_t* y, long R, int D, const DropArgs& dr, hipStream_t st);
void launch_dropout_mask(uint8_t* out, long row0, long R, int C, const DropArgs& dr, hipStream_t st);

// xent.hip
void launch_xent_fwd(const void* logits, bool bf16, const int64_t* labels, long R, long V, long ld, float* loss,
                     float* lse, long ignore_index, float smoothing, hipStream_t st);
void launch_xent_bwd(const void* logits, bool bf16, const int64_t* labels, const float* lse, const float* dscale,
                     bool per_row, long R, long V, long ld, void* dlogits, long ignore_index, float smoothing,
                     hipStream_t st);
// per-row loss and the label's rank among the first V columns (ties to the lower index; ignored rows: 0 and V)
void launch_xent_eval(const void* logits, bool bf16, const int64_t* labels, long R, long V, long ld, float* loss,
                      int* rank, long ignore_index, hipStream_t st);

// gemm.hip
int gemm_choose_splits(int M, int N, int K);
// accumulate-mode addend read from src (same layout as C) instead of C, elements with a clear bit in the packed
// mask (bit j of byte e = element 8e + j; null = all set) taken as zero (see Epi::addsrc in gemm.hip)
struct AddEpi {
  const uint16_t* src;
  const uint8_t* mask;
};
// gemm_short.hip: the short-K streaming GEMM (K in {64, 128, 256}, N % 128 == 0; see its header)
bool gemm_short_ok(int M, int N, int K, long lda, long ldc);
bool gemm_short_bnstats_ok(int M, int N, int K, bool dual);
// The BatchNorm-backward statistics a masked-addend data gradient can take in its epilogue: for the stored result g'
// of the BatchNorm y = relu(BN(x) + ...) whose packed ReLU bits are `mask`, g = mask ? g' : 0 and
//   sums[r][0][c] += sum g,  sums[r][1][c] += sum g (x - mean)   (r = the block's replica of kConvStatReplicas)
// and for a second BatchNorm fed by the same masked gradient (x2: sums2[r][1][c] += sum g (x2 - mean2)).
// The BatchNorm-backward sums a data-gradient epilogue accumulates for the non-residual BatchNorm + ReLU
// z = relu(BN(x)) that produced the convolution's input: g = relu_on(x) ? dx : 0 (the forward's ReLU decision, from
// gamma / beta / mean / invstd), sums[r][0][c] += sum g, sums[r][1][c] += sum g (x - mean). sums == nullptr: off.
struct BnBwdSums {
  const uint16_t* x = nullptr;
  const float* gamma = nullptr;
  const float* beta = nullptr;
  const float* mean = nullptr;
  const float* invstd = nullptr;
  float* sums = nullptr;
  // mask kind (a residual BatchNorm's packed ReLU bits instead of the affine ReLU decision): the row-remapped
  // accumulating data gradient's correction (gemm.hip TileEpi::LeanBnBwd, sub-grid rows); gamma / beta / invstd unused
  const uint8_t* mask = nullptr;
  // mask kind, the two-BatchNorm form (a ResNet downsample block's output: bn3 and the downsample BN share g):
  // sums2[.][1] += sum g (x2 - mean2) (identity-row path only)
  const uint16_t* x2 = nullptr;
  const float* mean2 = nullptr;
  float* sums2 = nullptr;
};
struct GemmShortBnStats {
  const uint16_t* x = nullptr;
  const uint8_t* mask = nullptr;
  const float* mean = nullptr;
  float* sums = nullptr;
  const uint16_t* x2 = nullptr;
  const float* mean2 = nullptr;
  float* sums2 = nullptr;
};
void launch_gemm_short(const uint16_t* A, const uint16_t* B, long ldb, bool b_mn, uint16_t* C, const uint16_t* add,
                       const uint8_t* mask, const float* xf, float* stats, int M, int N, int K, int epi,
                       hipStream_t st, const GemmShortBnStats* bst = nullptr);
void launch_gemm_dgrad_bnstats(const uint16_t* A, const uint16_t* B, uint16_t* C, int M, int N, int K,
                               const BnBwdSums& bb, hipStream_t st, bool accumulate = false,
                               const uint16_t* add_src = nullptr, const uint8_t* add_mask = nullptr);
// Which form of the tile kernel (gemm.hip TileEpi, "+A" / "+B" with an operand normalized on load) a launch described
// by plain values takes: the chooser every launch goes through, for tests without a GPU. Throws as the launch would.
struct TileFormQuery {
  const char* pair = "KK";  // operand sources: KK KM MK MM ConvK ConvGK MWg (gemm.hip Pair)
  int wm = 2;               // 2: 128 x 128 tiles, 4: 256 x 64
  int N = 128, splits = 1;
  int xuse = 0;             // the launch's XForm: 0 none, 1 normalize on load, 2 the inference scale
  long ldc = 128;
  int out_f32 = 0, mode = 0, act = 0;
  // which Epi pointers are set (rst: a sub-grid output), and whether c / pre are 16-B aligned
  bool bias = false, pre = false, stats = false, rst = false, addsrc = false, addmask = false, bb_sums = false,
       bb_mask = false, c_aligned = true, pre_aligned = true;
};
const char* gemm_tile_form(const TileFormQuery& q);
void launch_gemm(const uint16_t* A, long lda, bool a_kmajor, const uint16_t* B, long ldb, bool b_kmajor, void* C,
                 long ldc, bool c_f32, int M, int N, int K, const float* bias, int act, uint16_t* pre, int mode,
                 float alpha, int splits, float* ws, hipStream_t st, const AddEpi* add = nullptr,
                 const float* xform_b = nullptr, int xform_c = 0);
// out = bit ? src : 0 per element (bf16, n % 8 == 0; mask packed as above)
void launch_mask_apply(const uint16_t* src, const uint8_t* mask, uint16_t* out, long n, hipStream_t st);
long gemm_splitk_workspace(int M, int N, int splits);  // fp32 elements of the split-K slab workspace
// conv3x3.hip: staged-window 3 x 3 / stride-1 / pad-1 NHWC convolution (optional BN + ReLU on load: xform =
// fp32 [2][C] scale | shift), bf16 output, optional BN statistics [kConvStatReplicas][2][K]
bool conv3x3_eligible(int H, int W, int C, int K, int R, int S, int stride, int pad, int dil);
void launch_conv3x3(const uint16_t* x, const uint16_t* w, uint16_t* y, float* stats, const float* xform, int N,
                    int H, int W, int C, int K, hipStream_t st,
                    const BnBwdSums* bsums = nullptr);
// gemm256.hip: 256 x 256-tile, 8-wave phased MFMA GEMM for the large (transformer) products
bool gemm256_eligible(int M, int N, int K, bool a_kmajor, bool b_kmajor);
// split count for the tall-K fp32 products on the 256 x 256 kernel (1 = none)
int gemm256_choose_splits(int M, int N, int K);
// gemm256.hip: data gradient fused with the backward of the activation that produced the GEMM's input (4-wave kernel)
bool gemm_w4_dact_ok(int M, int N, int K, long lda, long ldb, long ldc);
long gemm_w4_dact_part_floats(int M, int N);
void launch_gemm_w4_dact(const uint16_t* A, long lda, const uint16_t* B, long ldb, uint16_t* C, long ldc, int M, int N,
                         int K, const uint16_t* pre, int act, float* part, float* db, bool db_accumulate,
                         float* sk_slabs, int* sk_sync, hipStream_t st);
// the down-projection data gradient fused with the SwiGLU backward: dgu [M][2F] (gemm256.hip copy_out_x ACT = -3)
bool gemm_w4_swiglu_ok(int M, int F, int K, long lda, long ldb);
void launch_gemm_w4_swiglu_bwd(const uint16_t* A, long lda, const uint16_t* B, long ldb, uint16_t* dgu,
                               const uint16_t* gu, int M, int F, int K, int blk, float* sk_slabs, int* sk_sync,
                               hipStream_t st);
bool gemm_w4_stats_ok(int M, int N, int K);
bool gemm_w4_dgrad_bnstats_ok(int M, int N, int K);
void launch_gemm_w4_dgrad_bnstats(const uint16_t* A, const uint16_t* B, uint16_t* y, int M, int N, int K,
                                  const uint16_t* x, const float* tab, float* sums, float* sk_slabs, int* sk_sync,
                                  hipStream_t st);
void launch_gemm_w4_stats(const uint16_t* A, long lda, const uint16_t* B, long ldb, uint16_t* y, int M, int N, int K,
                          float* stats, float* sk_slabs, int* sk_sync, hipStream_t st);
// gemm256.hip: a 3x3 / pad-1 / dilation-1 convolution (stride 1 or 2) as an implicit GEMM on the 4-wave kernel, its A
// rows gathered from the NHWC x [N][H][W][C] (ConvGather): y [N][Ho][Wo][K] = conv(x, w [K][3][3][C]). A stride-1 data
// gradient is the same call on dy with conv_dgrad_wtrans(w). One epilogue at most: `stats` (BnStats of the stored y,
// zeroed [kConvStatReplicas][2][K]) or bn_x / bn_tab / bn_sums (BnBwdSums, the operands of
// launch_gemm_w4_dgrad_bnstats); neither: the plain store. conv3x3_w4_ok is the contract (C % 64, K % 256, whole
// 256-row tiles, x below 2^31 elements); conv3x3_w4_use the policy -- $K8S_AMD_CONV3X3_W4 (0: off, read per call), a
// chip-filling grid and the shapes where the route measured faster than the kernels it replaces.
struct Gemm256Plan;
bool conv3x3_w4_ok(int N, int H, int W, int C, int K, int stride);
bool conv3x3_w4_use(int N, int H, int W, int C, int K, int stride, bool dgrad);
Gemm256Plan conv3x3_w4_plan(int N, int H, int W, int C, int K, int stride);  // its stream-K tail, for the workspace
void launch_conv3x3_w4(const uint16_t* x, const uint16_t* w, uint16_t* y, int N, int H, int W, int C, int K,
                       int stride, float* stats, const uint16_t* bn_x, const float* bn_tab, float* bn_sums,
                       float* sk_slabs, int* sk_sync, hipStream_t st);
// ... and its weight gradient dw [K][3][3][C] fp32 (+)= dy^T . im2col(x) with gathered B rows: C % 256 == 0 (a 256-column
// tile lies inside one tap), K % 256 == 0, N Ho Wo % 64 == 0; the tall-K split (conv3x3_w4_wgrad_splits > 1) goes
// through `ws` (conv3x3_w4_wgrad_workspace floats) and splitk_reduce. _use: the switch, and a chip-filling grid.
bool conv3x3_w4_wgrad_ok(int N, int H, int W, int C, int K, int stride);
bool conv3x3_w4_wgrad_use(int N, int H, int W, int C, int K, int stride);
int conv3x3_w4_wgrad_splits(int N, int H, int W, int C, int K, int stride);
long conv3x3_w4_wgrad_workspace(int N, int H, int W, int C, int K, int stride);
void launch_conv3x3_w4_wgrad(const uint16_t* x, const uint16_t* dy, float* dw, int N, int H, int W, int C, int K,
                             int stride, bool accumulate, float* ws, hipStream_t st);
bool gemm_w4_rope_ok(int M, int N, int K, long lda, long ldb, int rot_cols);
void launch_gemm_w4_rope(const uint16_t* A, long lda, const uint16_t* B, long ldb, uint16_t* y, int M, int N, int K,
                         const int* pos, const float* table, int rot_cols, float* sk_slabs, int* sk_sync,
                         hipStream_t st);
bool gemm_w4_swiglu_fwd_ok(int M, int F, int K, long lda, long ldb);
void launch_gemm_w4_swiglu_fwd(const uint16_t* A, long lda, const uint16_t* B, long ldb, uint16_t* gu, uint16_t* h,
                               int M, int F, int K, float* sk_slabs, int* sk_sync, hipStream_t st);
// stream-K tail plan (gemm256.hip): tiles [full, tiles) are split sk ways along K (sk == 1: none), kps deep each
struct Gemm256Plan {
  int tiles, full, sk, kps;
};
Gemm256Plan gemm256_plan(int M, int N, int K);
long gemm256_sk_slab_floats(const Gemm256Plan& p);  // fp32 partial slabs the stream-K tail needs
long gemm256_sk_sync_ints(const Gemm256Plan& p);    // zeroed ints (ticket + flags) it needs; left zeroed after
void launch_gemm256(const uint16_t* A, long lda, bool a_kmajor, const uint16_t* B, long ldb, bool b_kmajor, void* C,
                    long ldc, bool c_f32, int M, int N, int K, const float* bias, int act, uint16_t* pre,
                    bool accumulate, float alpha, hipStream_t st, int splits = 1, float* ws = nullptr,
                    float* sk_slabs = nullptr, int* sk_sync = nullptr);
// Output written to the (a, b) parity sub-grid of an H x W image: GEMM row (n, i, j) -> (n, i*stride+a,
// j*stride+b). Used for stride-s data gradients decomposed by output parity (ops/conv.py _dgrad_strided_hip).
struct SubGrid {
  int H, W, stride, a, b;
};
void launch_conv_fwd(const uint16_t* x, const uint16_t* w, void* y, bool y_f32, int N, int H, int W, int C, int K,
                     int R, int S, int stride, int pad, int dil, int Ho, int Wo, const float* bias, int act,
                     int mode, float* stats, hipStream_t st, const SubGrid* sg = nullptr, const float* xform = nullptr,
                     const BnBwdSums* bb = nullptr);
// Inference convolution + folded BatchNorm (+ residual) (+ ReLU) on the tile kernel (gemm.hip TileEpi::LeanInfer):
//   y = act(bf16(conv(x, w) * scale[k] + shift[k]) + res), scale / shift fp32 [K], res bf16 with y's layout or null.
// C % 8 == 0, K % 8 == 0, dilation 1, 16-B aligned pointers; throws outside that contract.
void launch_conv_infer(const uint16_t* x, const uint16_t* w, uint16_t* y, int N, int H, int W, int C, int K, int R,
                       int S, int stride, int pad, int Ho, int Wo, const float* scale, const float* shift,
                       const uint16_t* res, bool relu, hipStream_t st);
// xform (here and in launch_gemm / launch_wgrad_stream): fp32 [2][C] BatchNorm (scale | shift): the activation
// operand x is consumed as relu(x * scale + shift), normalised as it is loaded (gemm.hip XForm)
void launch_conv_wgrad(const uint16_t* x, const uint16_t* dy, float* dw, int N, int H, int W, int C, int K, int R,
                       int S, int stride, int pad, int dil, int Ho, int Wo, int splits, bool accumulate, float* ws,
                       hipStream_t st, const float* xform = nullptr);
// wgrad_stream.hip: tall-K weight gradient (few output tiles, millions of rows), fp32 atomics into dw
bool wgrad_stream_eligible(int N, int Ho, int Wo, int C, int K, int R, int S);
void launch_wgrad_stream(const uint16_t* x, const uint16_t* dy, float* dw, int N, int H, int W, int C, int K, int R,
                         int S, int stride, int pad, int Ho, int Wo, bool accumulate, hipStream_t st);
// bwd1x1_fused.hip: the whole backward of a 1x1 / stride-1 convolution whose input is relu(BN(x)) normalised on load,
// in one pass over gy [M][K] and x [M][C]: dz = gy . w (bf16), dw [K][C] fp32 (+)= gy^T . relu(bf16(x scale + shift))
// (xform = fp32 [2][C] scale | shift), and the BatchNorm-backward sums of dz (as BnBwdSums, relu kind) into the zeroed
// sums [kConvStatReplicas][2][C]. (C, K) = (64, 256) or (128, 512), M < 2^31; dw is zeroed first unless accumulating.
// bn3 (optional): gy is the incoming dy of the residual BatchNorm that produced the convolution's output, and the kernel
// applies that BatchNorm's backward as it loads: its gy tile is bf16(fma(sc, mask ? dy : 0, fma(B, x3, D))), the bits
// bn_bwd_apply_kernel would have written, never stored. x3 [M][K] bf16, mask [M][K / 8] packed ReLU bits, params fp32
// [sc | B | D] (3K or more, launch_bn_bwd_params).
struct Bwd1x1Bn3 {
  const uint16_t* x3 = nullptr;
  const uint8_t* mask = nullptr;
  const float* params = nullptr;
};
// fin (optional, (C, K) = (64, 256) only): the final form, for a convolution whose input is a stored tensor and whose
// data gradient is the second into it (ResNet's stage-1 downsample convolution on the stem pool's output). x is the dW
// operand as stored (xform, gamma, beta, mean, invstd null); out = bf16(bf16(gy . w) + addend), the rounding of the tile
// kernel's accumulating epilogue, is written over addend (dz == addend); the sums are the pool kind's over the stored sum: g = bit ? out : 0, sums[r][0] += g,
// sums[r][1] += g (winner_x - winner_mean), winner_x [M][64] bf16 and winner_bits [M][8] the pooled forward's window
// winners and their packed ReLU bits. With bn3 the gy tile is formed on load as above.
struct Bwd1x1Final {
  const uint16_t* addend = nullptr;
  const uint16_t* winner_x = nullptr;
  const uint8_t* winner_bits = nullptr;
  const float* winner_mean = nullptr;
  float* dw_partials = nullptr;  // bwd1x1_final_workspace floats: dW's per-workgroup slabs, summed in order into dw
};
bool bwd1x1_fused_ok(long M, int C, int K);
bool bwd1x1_final_ok(long M, int C, int K);
long bwd1x1_final_workspace(long M, int C, int K);
void launch_bwd1x1_fused(const uint16_t* gy, const uint16_t* x, const uint16_t* w, const float* xform,
                         const float* gamma, const float* beta, const float* mean, const float* invstd, uint16_t* dz,
                         float* dw, float* sums, long M, int C, int K, bool accumulate, hipStream_t st,
                         const Bwd1x1Bn3* bn3 = nullptr, const Bwd1x1Final* fin = nullptr);
// conv1_fused.hip: the whole backward of the 1x1 / stride-1 convolution that opens a ResNet identity bottleneck (N -> W
// channels, (W, N) = (64, 256) or (128, 512), M < 2^31) with the apply pass of the BatchNorm + ReLU behind it formed on
// load, in one pass: dx1 = bf16(fma(sc, relu_on(x1) ? dz1 : 0, fma(B, x1, D))) (params fp32 [sc | B | D | shift], 4W,
// launch_bn_bwd_params with relu_x) is never stored; dx [M][N] = bf16(bf16(dx1 . w) + (abit ? dy : 0)), w [W][N];
// sums [kConvStatReplicas][2][N] (zeroed) += sum g, sum g (x3 - mean), g = bit ? dx : 0 (GemmShortBnStats, one
// BatchNorm); dw [W][N] fp32 (+)= dx1^T . xin through per-walker slabs summed in order (no atomics).
struct Conv1Fused {
  const uint16_t *dz1 = nullptr, *x1 = nullptr;  // [M][W]
  const float* params = nullptr;
  const uint16_t *w = nullptr, *xin = nullptr;   // [W][N], [M][N]
  const uint16_t* dy = nullptr;                  // the masked addend [M][N] and its packed bits [M][N / 8]
  const uint8_t* abits = nullptr;
  const uint16_t* x3 = nullptr;                  // the BatchNorm of the sums: input, packed ReLU bits, mean
  const uint8_t* bits = nullptr;
  const float* mean = nullptr;
  uint16_t* dx = nullptr;
  float *sums = nullptr, *dw = nullptr;
  float* dw_partials = nullptr;  // conv1_fused_workspace floats
};
bool conv1_fused_ok(long M, int W, int N);
long conv1_fused_workspace(long M, int W, int N);
void launch_conv1_fused(const Conv1Fused& c, long M, int W, int N, bool accumulate, hipStream_t st);
void launch_conv_dgrad_wtrans(const uint16_t* w, uint16_t* w2, int K, int R, int S, int C, hipStream_t st);
// per-output-parity sub-weights of a stride-s dgrad (up to 16 parities x 16 taps), packed at off[p]
struct DgradTaps {
  int n[16];
  long off[16];
  int rs[16][16];
};
void launch_conv_dgrad_wsub(const uint16_t* w, uint16_t* out, int K, int RS, int C, const DgradTaps& taps, int np,
                            hipStream_t st);

// elementwise.hip
void launch_swiglu_fwd(const uint16_t* gu, uint16_t* y, long T, int F, int blk, hipStream_t st);
void launch_swiglu_bwd(const uint16_t* gu, const uint16_t* dy, uint16_t* dgu, long T, int F, int blk, hipStream_t st);
void launch_rope(uint16_t* x, long ld, const int* pos, const float* table, long T, int H, int D, bool inverse,
                 hipStream_t st);
void launch_gelu_bwd(const uint16_t* dy, const uint16_t* pre, uint16_t* dx, long n, hipStream_t st);
void launch_relu_bwd(const uint16_t* dy, const uint16_t* y, uint16_t* dx, long n, hipStream_t st);
int colsum_workspace_floats(long R, int C);
void launch_colsum(const uint16_t* x, long R, int C, float* work, float* out, bool accumulate, hipStream_t st);
// the fold of P partial rows of column sums (colsum_fold_kernel)
// (P > 256: two levels, overwriting part)
void launch_colsum_fold(float* part, int P, int C, float* out, bool accumulate, hipStream_t st);
// the first level of that fold alone: the sum of rows [g gs, (g + 1) gs) written over row g gs
void launch_colsum_group(float* part, int P, int C, int gs, hipStream_t st);
// g = dy * act'(pre) (1 ReLU, pre = its output; 2 GELU(tanh), pre = the pre-activation) and out = column sums of g
void launch_act_bwd_colsum(int act, const uint16_t* dy, const uint16_t* pre, uint16_t* g, long R, int C, float* work,
                           float* out, bool accumulate, hipStream_t st);

// ---- K5 flash attention (attention.hip). q [B,Sq,Hq,D], k/v [B,Sk,Hkv,D] (strided, last dim contiguous)
// what a call masks beyond causal / kv_lens: at most one of dropout on the probabilities, a document mask, a span mask
enum class AttnMask { Plain, Drop, Doc, Span };
struct AttnFwdArgs {
  const uint16_t *q, *k, *v;
  uint16_t* o;
  float* lse;          // [B, Hq, lse_ld]: m + log2(l) in the exp2 domain (scores scaled by scale*log2(e))
  const int* kv_lens;  // [B] or null
  long sqb, sqs, sqh, skb, sks, skh, svb, svs, svh, sob, sos, soh;
  long lse_ld;         // row stride of lse (Sq rounded up to 64)
  int B, Sq, Sk, Hq, Hkv, causal;
  float scale_log2;
  // dropout on the probabilities (AttnMask::Drop, the shapes flash_plan takes): row = (b * Hq + h) * Sq + q, col = key
  DropArgs drop;
  // What is masked beyond causal / kv_lens, and the one table pair of the Doc and Span kinds: int32 [B, Sq], both or
  // neither; device data the kernels clamp before use (MaskRow).
  // Doc (causal self-attention only): query i sees the keys mask_lo[i] <= j <= i, and mask_hi[j] is one past the last
  // query that sees key j. The forward and the dQ kernel read lo, the dK/dV kernel hi.
  // Span (non-causal self-attention at D = 64 only): query i sees the keys mask_lo[i] <= j < mask_hi[i]. Every kernel
  // reads both. span_tile: keys per tile of the Span forms, 64 or 128 (0: the plan's default).
  AttnMask mask = AttnMask::Plain;
  const int* mask_lo = nullptr;
  const int* mask_hi = nullptr;
  int span_tile = 0;
};
struct AttnBwdArgs {
  const uint16_t *q, *k, *v, *dO;
  const float* lse;
  float* delta;       // [B, Hq, lse_ld] scratch
  uint16_t* dq;       // [B, Sq, Hq, D] at strides (sgqb, sgqs, sgqh)
  uint16_t *dk, *dv;  // [B, Sk, Hkv, D] at strides (sgkb, sgks, sgkh) / (sgvb, sgvs, sgvh)
  const int* kv_lens;
  long sqb, sqs, sqh, skb, sks, skh, svb, svs, svh, sdb, sds, sdh;
  // output strides: a packed [B*S, (Hq + 2*Hkv) * D] gradient of a fused QKV projection is written in place
  long sgqb, sgqs, sgqh, sgkb, sgks, sgkh, sgvb, sgvs, sgvh;
  long lse_ld;
  int B, Sq, Sk, Hq, Hkv, causal;
  float scale_log2, scale;
  // dK/dV split into dkv_split chunks per key block (FlashPlan): fp32 partials [dkv_split][2][B][Hkv][Sk][D]
  int dkv_split = 1;
  float* dkv_ws = nullptr;
  // one-block short-sequence form only (FlashPlan::Bwd::one_block): per-batch column sums of the packed QKV gradient,
  // fp32 [B][cpart_ld] (the projection's bias gradient once folded over B)
  float* cpart = nullptr;
  int cpart_ld = 0;
  DropArgs drop;  // as the forward's
  // dropout on the three-kernel form: the queries' row keys, [B, Hq, lse_ld] scratch next to delta (written by the
  // row-key kernel from the device [seed, step] pair, read by the dK/dV and dQ kernels)
  uint32_t* rowkey = nullptr;
  AttnMask mask = AttnMask::Plain;  // as the forward's, with its table pair
  const int* mask_lo = nullptr;
  const int* mask_hi = nullptr;
  int span_tile = 0;
};

// Which kernels run for a shape, and whether the flash kernels take it at all: the one place that knows the tile
// choice (128-key steps at D = 64 from 1024 tokens on; the forward picks by Sk, the backward by Sq), the one-tile
// forward, the one-block backward, the QS = 2 dQ, the dK/dV split and the Span forms' index limits. A pure host
// function of the shape (and planner_cus()); the launchers, the binding and Python all read it.
struct FlashPlan {
  bool ok = true;
  const char* reason = "";  // one sentence when !ok
  struct Fwd {
    int tile = 64, nb = 2;  // keys per tile; stage buffers (1: the one-tile form, every key in one 128-key tile)
  } fwd;
  struct Bwd {
    bool one_block = false;     // flash_bwd_short_kernel: the whole backward of a (batch, head) in one block
    int tile = 64, qs = 1;      // (three kernels) queries / keys per step; 16-query sets per dQ wave
    int dkv_split = 1;          // dK/dV chunks per key block (above 1: fp32 partials and the reduce kernel)
    bool needs_rowkey = false;  // dropout on the three-kernel form: the row-key table beside delta
  } bwd;
};
// max_token_stride: the largest token stride of any operand, in elements. want_dbias: the caller asks for the packed
// projection's bias gradient (the one-block kernel's column partials).
FlashPlan flash_plan(int D, long B, long Sq, long Sk, long Hq, long Hkv, bool causal, bool has_kv_lens, AttnMask mask,
                     int span_tile, long max_token_stride, bool want_dbias);
// the plan of a filled argument block (sos: o's token stride)
FlashPlan flash_plan(const AttnFwdArgs& a, int D);
FlashPlan flash_plan(const AttnBwdArgs& a, int D, long sos, bool want_dbias);
// ResNet stem BatchNorm + ReLU + 3x3 / s2 / p1 max pool, fused (batchnorm.hip): forward from the conv's epilogue sums
// (params = fp32 [2][C] scale | shift, idx = winner byte per pooled element); backward into dx of the conv output
// (params = fp32 [4][C] workspace, work = pool_bn_workspace_floats(C))
void launch_bn_relu_maxpool_fwd(const uint16_t* x, const float* gamma, const float* beta, const float* sums, int nrep,
                                float* save_mean, float* save_invstd, float* run_mean, float* run_var, float* params,
                                uint16_t* y, uint8_t* idx, int N, int H, int W, int C, float eps, float momentum,
                                hipStream_t st, uint16_t* xarg = nullptr, uint8_t* ybits = nullptr);
int pool_bn_workspace_floats(int C);
// s.sums (with nrep) given: the final and apply passes only, else s.work = pool_bn_workspace_floats(C)
void launch_pool_bn_bwd(const uint16_t* dpool, const uint8_t* idx, int nrep, const BnBwdSide& s, int N, int H, int W,
                        int C, hipStream_t st);

void launch_flash_fwd(const AttnFwdArgs& a, int D, hipStream_t st);
void launch_flash_bwd(const AttnBwdArgs& a, int D, const uint16_t* o, long sob, long sos, long soh, hipStream_t st);

// ---- embedding.hip: sum of up to 3 table gathers (fwd) / fp32 atomic scatter-add into gradient slots (bwd)
struct EmbTable {
  const uint16_t* w;   // [V][D] bf16 table (forward)
  float* g;            // [V][D] fp32 gradient (backward; accumulated into)
  const int64_t* ids;  // [T] row ids, or null: row = token % S (position table)
  int V;
};
void launch_embed_fwd(const EmbTable* tabs, int ntab, int T, int D, int S, uint16_t* out, hipStream_t st);
void launch_embed_bwd(const EmbTable* tabs, int ntab, int T, int D, int S, const uint16_t* g, hipStream_t st);

// ---- NHWC average pooling over H*W (pool.hip): y[n][c] = mean_hw x[n][hw][c] (fp32 accumulate, bf16 out)
void launch_avgpool_fwd(const uint16_t* x, uint16_t* y, int N, int HW, int C, hipStream_t st);
void launch_avgpool_bwd(const uint16_t* dy, uint16_t* dx, int N, int HW, int C, hipStream_t st);

// ---- stem.hip: 7x7 / stride-2 stem as a 4x4 conv over the 2x2 space-to-depth image (16 channels)
void launch_stem_s2d_input(const uint16_t* x, int N, int H, int W, int Cin, int pad, uint16_t* out, hipStream_t st);
void launch_stem_w_s2d(const uint16_t* w7, int K, int R, int Cw, uint16_t* w4, hipStream_t st);
// the s2d stem conv (K = 64, 4x4 taps, 16 channels) LDS-tiled, BN statistics into stats [kConvStatReplicas][2][64]
bool stem_conv_fwd_ok(int K, int R, int C, int Wo);
void launch_stem_conv_fwd(const uint16_t* xs, const uint16_t* w4, uint16_t* y, float* stats, int N, int Hs, int Ws,
                          hipStream_t st);
// out[i] (+)= sum over `splits` fp32 slabs of mn elements (gemm.hip)
void splitk_reduce(const float* ws, int splits, long mn, float* out, bool accumulate, hipStream_t st);
// LDS-tiled 3x3 / s1 / p1 weight gradient (wgrad_tile.hip), C == K in 64 pieces; ws = wgrad3x3_tiled_workspace floats
bool wgrad3x3_tiled_ok(int C, int K, int R, int S, int stride, int pad, int W);
int wgrad3x3_tiled_blocks(int N, int H, int W, int C);
long wgrad3x3_tiled_workspace(int N, int H, int W, int C);
void launch_wgrad3x3_tiled(const uint16_t* x, const uint16_t* dy, float* ws, float* dw, int N, int H, int W, int C,
                           bool accumulate, hipStream_t st, const float* xform = nullptr);
// the s2d stem weight gradient (LDS-tiled, persistent blocks; ws = stem_wgrad_blocks(N, Hs) x 64 x 256 fp32 partials)
int stem_wgrad_blocks(int N, int Hs);
void launch_stem_wgrad(const uint16_t* xs, const uint16_t* dy, float* ws, float* dw4, int N, int Hs, int Ws,
                       hipStream_t st);
void launch_stem_dw_s2d(const float* dw4, int K, int R, int Cw, float* dw7, hipStream_t st);

// ---- augment.hip: a dataset batch in one pass -- gather by the int32 table [N][6] (src index, y0, x0, h, w, flip),
// crop or bilinear resize to S x S, flip, bf16(fmaf(u8, a_c, b_c)), written as the stem's input ([N][S][S][8], or
// with s2d the [N][S/2+3][S/2+3][16] image of launch_stem_s2d_input at pad 3). src uint8 [M][Hs][Ws][3].
struct AugNorm {
  float a[3], b[3];  // 1 / std_c, -mean_c / std_c
};
void launch_augment(const uint8_t* src, const int* table, int N, int M, int Hs, int Ws, int S, const AugNorm& nm,
                    bool s2d, uint16_t* out, hipStream_t st);

// ---- token_batch.hip: a token batch in one launch. src: the token array, uint16 (u16) or int32 [Tn]; all outputs
// int64. mlm_batch: table int64 [N][6] rows (a0, la, b0, lb, n, ord) -> ids / types [N][S], labels / positions
// [N][P] of a BERT pretraining batch (1 <= P <= S <= 512); causal_batch: starts int64 [N] -> ids = src[start + j],
// labels = src[start + j + 1], [N][S]. Every source index is clamped into [0, Tn).
struct TokSpecial {
  int pad, cls, sep, mask;
};
void launch_mlm_batch(const void* src, bool u16, long Tn, const long* table, int N, int S, int P, uint32_t vocab,
                      const TokSpecial& sp, uint64_t seed, int stream, long* ids, long* types, long* labels,
                      long* positions, hipStream_t st);
// the same samples back to back in one stream of Tt rows (Tt % 128 == 0, Tt < 2^31): cu int64 [N + 1] (device) the
// samples' first rows; ids / types / pos int64 [Tt], labels / rows int64 [N, P], cls_rows int64 [N], lo / hi int32 [Tt]
void launch_mlm_batch_unpadded(const void* src, bool u16, long Tn, const long* table, const long* cu, long Tt, int N,
                               int S, int P, uint32_t vocab, const TokSpecial& sp, uint64_t seed, int stream, long* ids,
                               long* types, long* pos, long* labels, long* rows, long* cls_rows, int* lo, int* hi,
                               hipStream_t st);
void launch_causal_batch(const void* src, bool u16, long Tn, const long* starts, int N, int S, long* ids, long* labels,
                         hipStream_t st);
// causal_batch with document boundaries: doc_tok int64 [Dn + 1] ascending token offsets of the documents (device),
// abs_starts the windows' positions in the split; also writes int32 [N, S] lo, hi (the document of each token, as
// row indices) and pos (the token's position inside its document)
void launch_causal_doc_batch(const void* src, bool u16, long Tn, const long* starts, const long* abs_starts,
                             const long* doc_tok, long Dn, int N, int S, long* ids, long* labels, int* lo, int* hi,
                             int* pos, hipStream_t st);

// ---- NHWC max pooling (pool.hip): idx = winning window position per output element (uint8)
void launch_subsample_nhwc(const uint16_t* x, uint16_t* y, int N, int H, int W, int C, int s, hipStream_t st);
void launch_maxpool_fwd(const uint16_t* x, uint16_t* y, uint8_t* idx, int N, int H, int W, int C, int Ho, int Wo,
                        int k, int s, int p, hipStream_t st);
void launch_maxpool_bwd(const uint16_t* dy, const uint8_t* idx, uint16_t* dx, int N, int H, int W, int C, int Ho,
                        int Wo, int k, int s, int p, hipStream_t st);

// decode.hip: generation. linear_skinny: y[M, N] = x[M, K] . w[N, K]^T for 1 <= M <= 16, K % 64 == 0, N % 16 == 0
// (linear_skinny_ok); skinny_plan: its K split, a function of (N, K) alone -- `part` holds nsplit fp32 [M, N] partials
// when nsplit > 1 and is not read otherwise.
struct SkinnyPlan {
  int kc = 0;      // k per chunk, a multiple of 64
  int nsplit = 1;  // chunks
};
bool linear_skinny_ok(long M, long N, long K);
SkinnyPlan skinny_plan(long N, long K);
void launch_linear_skinny(const uint16_t* x, const uint16_t* w, uint16_t* y, float* part, int M, int N, int K,
                          hipStream_t st);
// token s of row b of qkv [B * S, (Hq + 2 Hkv) * D] -> position clamp(start[b] + s, 0, Smax - 1) of the bf16 caches
// [B, Hkv, Smax, D]; start: device int32 [B]
void launch_kv_append(const uint16_t* qkv, uint16_t* ck, uint16_t* cv, const int* start, int B, int S, int Hq, int Hkv,
                      int D, int Smax, hipStream_t st);
// one new token per row: q [B, Hq, D] with row stride ldq (elements, a multiple of 8), caches [B, Hkv, Smax, D], lens device int32 [B] (clamped into [1, Smax]), out
// [B, Hq * D]. Keys in chunks of kDecodeChunk; nchunks chunks are launched (every row's len <= nchunks * kDecodeChunk
// is the caller's to ensure; a longer row attends to that many keys); workspaces fp32 ws_ml [B, Hkv, nchunks, G, 2]
// and ws_o [B, Hkv, nchunks, G, D], G = Hq / Hkv <= 16.
constexpr int kDecodeChunk = 256;
void launch_decode_attention(const uint16_t* q, long ldq, const uint16_t* ck, const uint16_t* cv, const int* lens, float* ws_ml,
                             float* ws_o, uint16_t* out, int B, int Hq, int Hkv, int D, int Smax, int nchunks,
                             float scale, hipStream_t st);

}  // namespace k8s_amd
